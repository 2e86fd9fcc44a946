/*
 * mla_hip.h -- C ABI of libmla_hip.so: the MI355X (gfx950) kernels of the MLA
 * alternating-unimodal training step (reference: main.py:419-476 and the modules it calls).
 *
 * The reference has no FFI: its "operator interface" for this path is the set of implicit ATen ops
 * that nn.Conv2d / nn.BatchNorm2d / nn.MaxPool2d / F.adaptive_avg_pool / nn.Linear /
 * nn.CrossEntropyLoss / GSPlugin.before_update / torch.optim.SGD trigger.  Each entry point below
 * replaces one of those op groups and cites the reference line that triggers it.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no torch types; nothing is allocated, freed or synchronised;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); kernels are enqueued on it;
 *   - activations are NHWC fp32 ("pixel-major": [N][H][W][C]); conv weights are HWIO fp32
 *     ([KH][KW][Cin][Cout]); the Python boundary converts from/to the reference's NCHW / OIHW;
 *   - return 0 on success, a negative mla_status on error (never throws, never aborts).
 */
#ifndef MLA_HIP_H
#define MLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum mla_status {
  MLA_OK = 0,
  MLA_ERR_INVALID_ARG = -1,   /* shape/pointer the kernels do not support */
  MLA_ERR_WORKSPACE = -2,     /* workspace too small */
  MLA_ERR_LAUNCH = -3         /* hipGetLastError() != hipSuccess after launch */
};

/* Library/ABI version and a human-readable description of the last error on this thread. */
int mla_abi_version(void);
const char* mla_last_error(void);

/* ---- layout (boundary) ---------------------------------------------------------------------- */
/* (B,C,T,H,W) video -> (B*T,H,W,C) frames.  Replaces backbone.py:144-147 permute+contiguous+view. */
int mla_video_to_nhwc(const float* src, float* dst, int B, int C, int T, int H, int W, void* stream);
/* generic NCHW <-> NHWC (tests / state import) */
int mla_nchw_to_nhwc(const float* src, float* dst, int N, int C, int H, int W, void* stream);
int mla_nhwc_to_nchw(const float* src, float* dst, int N, int C, int H, int W, void* stream);

/* ---- convolution: nn.Conv2d (backbone.py:4-12, 79-83, 28, 31, 127) --------------------------- */
/* Implicit-GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).
 * bn_partial (nullable): if given, the epilogue also writes per-M-tile column sums and sums of
 * squares of y, layout [tiles][2][Cout]; *bn_tiles receives `tiles`.  Feed to mla_bn_finalize. */
/* measurement hook: force the fp32 kernels' tile 0..3 (128x128, 256x64, 64x64, 128x64) where Cout allows; -1 = automatic */
int mla_conv2d_f32_cfg(int cfg);
size_t mla_conv2d_fwd_partial_elems(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mla_conv2d_fwd(const float* x, const float* w_hwio, float* y,
                   int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                   float* bn_partial, int* bn_tiles, void* stream);

/* Input gradient (autograd of the above).  dx = dgrad(dy) [+ residual] [* (relu_src > 0)].
 * `residual` may alias `dx` (accumulate).  wt_ws: Cin*Cout*KH*KW floats of scratch (per-tap
 * transposed weights).  (H,W) are the INPUT dims of the forward conv. */
int mla_conv2d_dgrad(const float* dy, const float* w_hwio, float* dx,
                     int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                     const float* residual, const float* relu_src, float* wt_ws, void* stream);

/* Weight gradient: dw_hwio[kh][kw][ci][co] = sum_pixels x * dy.  Deterministic split-K:
 * partial slabs in `ws` (mla_conv2d_wgrad_ws_bytes) followed by an ordered reduce. */
size_t mla_conv2d_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mla_conv2d_wgrad(const float* x, const float* dy, float* dw_hwio,
                     int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- convolution, split-bf16 arithmetic (same nn.Conv2d sites as above) -------------------------
 * The same gather-GEMM with every fp32 operand split exactly into three bf16 terms and the six products
 * a_i*b_j (i+j <= 2) accumulated in fp32 on v_mfma_f32_32x32x16_bf16: fp32 in, fp32 out, error against
 * the exact sum of the same order as the fp32-MFMA entry points (dropped terms <= 2^-23 |a*b|), at 6/16 of
 * their MFMA cycles.  Weights are pre-split by mla_conv2d_wsplit into mla_conv2d_wsplit_bytes of scratch:
 * transposed = 1 for mla_conv2d_fwd_split, 0 for mla_conv2d_dgrad_split.  Cin, Cout multiples of 64
 * (the stem stays on mla_conv2d_fwd).  Other arguments as in mla_conv2d_fwd / mla_conv2d_dgrad.
 * mla_conv2d_split_terms(t) (t = 3, 6, 8; anything else only queries) selects the product set for
 * measurements; 6 is the default and the only set the parity tests bless. */
size_t mla_conv2d_wsplit_bytes(int Cin, int Cout, int KH, int KW);
int mla_conv2d_wsplit(const float* w_hwio, void* wsplit, int Cin, int Cout, int KH, int KW, int transposed, void* stream);
/* Batched form (one launch for all convs of a flat parameter buffer).  desc: n <= 4096 rows of 8 ints in DEVICE memory,
 * {w_off (floats from params), out_off (16-bit elements from wsplit), taps, Cin, Cout, transposed, first_block, 0} with
 * first_block the running sum of taps*ceil(Cin/32)*ceil(Cout/32); total_blocks = that sum over all rows. */
int mla_conv2d_wsplit_batch(const float* params, void* wsplit, const int* desc, int n, int total_blocks, void* stream);
int mla_conv2d_fwd_split(const float* x, const void* wsplit_t, float* y,
                         int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                         float* bn_partial, int* bn_tiles, void* stream);
int mla_conv2d_dgrad_split(const float* dy, const void* wsplit, float* dx,
                           int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                           const float* residual, const float* relu_src, void* stream);

/* Input gradient that also forms the reduction pass of the BatchNorm backward(s) consuming dx: for each request q (at most 2:
 * the BatchNorm before this convolution in the forward pass, and a downsample BatchNorm beside it) the epilogue writes the
 * per-tile column sums  sum dx  and  sum dx * (x_q - mean_q) * invstd_q  to partial_q[tile][2][Cin] (floats; size
 * mla_conv2d_dgrad_bn_partial_elems; *bn_tiles = number of tiles written), which mla_bn_bwd_from_partial then finalizes and
 * applies.  Saves re-reading dx and x in a separate reduction pass.  nreq = 0: identical to mla_conv2d_dgrad[_split]. */
typedef struct mla_bn_reduce_req {
  const float* x;        /* the BatchNorm's input (conv output), (N,H,W,Cin) like dx */
  const float* mean;     /* its saved batch mean / inverse standard deviation, (Cin) */
  const float* invstd;
  float* partial;        /* out */
} mla_bn_reduce_req;
size_t mla_conv2d_dgrad_bn_partial_elems(int N, int H, int W, int Cin);
int mla_conv2d_dgrad_bn(const float* dy, const float* w_hwio, float* dx, int N, int H, int W, int Cin, int Cout,
                        int KH, int KW, int stride, int pad, const float* residual, const float* relu_src, float* wt_ws,
                        const mla_bn_reduce_req* reqs, int nreq, int* bn_tiles, void* stream);
int mla_conv2d_dgrad_split_bn(const float* dy, const void* wsplit, float* dx, int N, int H, int W, int Cin, int Cout,
                              int KH, int KW, int stride, int pad, const float* residual, const float* relu_src,
                              const mla_bn_reduce_req* reqs, int nreq, int* bn_tiles, void* stream);
/* ... restricted to some output parity classes of a strided convolution (bit py * stride + px of class_mask; stride 1: bit 0),
 * with `residual` added only in the classes of residual_mask.  Lets the 1x1 / stride-2 downsample input gradient
 * (backbone.py:126-129) write just the one class it reaches, and the 3x3 / stride-2 conv1 beside it (backbone.py:28) accumulate
 * onto it there, instead of a full read-modify-write pass over dx in four launches.  (0xF, 0xF) = the plain entry points. */
int mla_conv2d_dgrad_classes(const float* dy, const float* w_hwio, float* dx, int N, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, const float* residual, const float* relu_src, float* wt_ws,
                             const mla_bn_reduce_req* reqs, int nreq, int* bn_tiles, int class_mask, int residual_mask,
                             void* stream);
int mla_conv2d_dgrad_split_classes(const float* dy, const void* wsplit, float* dx, int N, int H, int W, int Cin, int Cout,
                                   int KH, int KW, int stride, int pad, const float* residual, const float* relu_src,
                                   const mla_bn_reduce_req* reqs, int nreq, int* bn_tiles, int class_mask, int residual_mask,
                                   void* stream);
/* weight gradient on the same arithmetic (both operands split in the kernel); workspace and reduce as mla_conv2d_wgrad */
size_t mla_conv2d_wgrad_split_ws_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mla_conv2d_wgrad_split(const float* x, const float* dy, float* dw_hwio,
                           int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                           void* ws, size_t ws_bytes, void* stream);
/* measurement hook: 0 = per-tap weight-gradient kernel for every layer, 1 (default) = the persistent all-taps kernel
 * (transposing LDS reads) for the 64 -> 64 channel 3x3 / stride 1 convolutions; other values: query.  Returns the setting. */
int mla_conv2d_wgrad_tr(int on);
/* measurement / test hook: 0 = per-tap gather-GEMM for every layer, 1 (default; $MLA_CONV_PATCH overrides) = LDS-resident
 * input patch (conv_patch_split.hip) for the 3x3 / stride 1 / pad 1 forward and input-gradient launches whose grid fills the chip,
 * 2 = for all of them; other values: query.  Returns the setting. */
int mla_conv2d_patch(int on);
/* BatchNorm folded into the operands of the 64 -> 64 channel 3x3 / stride 1 / pad 1 convolutions (split arithmetic; conv2 of the layer1
 * BasicBlocks, models/backbone.py:38-46: conv1 -> bn1 -> relu -> conv2).  The consumers of a = relu(bn1(y1)) -- conv2's forward, conv2's weight
 * gradient and the ReLU mask of conv2's input gradient -- form it from y1 with the expression of mla_bn_apply, bit for bit, so `a` is
 * never written or read.  in_* / mask_*: per-channel BatchNorm parameters (training: batch statistics; evaluation: running statistics).
 * mla_conv2d_bnfold_supported: 1 where these entry points apply (they fail with MLA_ERR_INVALID_ARG elsewhere).
 *   mla_conv2d_fwd_split_bnin     = mla_conv2d_fwd_split   over relu(bn(x))
 *   mla_conv2d_wgrad_split_bnin   = mla_conv2d_wgrad_split over relu(bn(x))
 *   mla_conv2d_dgrad_split_bnmask = mla_conv2d_dgrad_split_bn with relu_src := relu(bn(reqs[0].x)) (gamma / beta given; mean / invstd: the request's) */
int mla_conv2d_bnfold_supported(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mla_conv2d_fwd_split_bnin(const float* x, const void* wsplit_t, float* y, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                              int stride, int pad, const float* in_mean, const float* in_invstd, const float* in_gamma, const float* in_beta,
                              float* bn_partial, int* bn_tiles, void* stream);
int mla_conv2d_wgrad_split_bnin(const float* x, const float* dy, float* dw_hwio, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                int stride, int pad, const float* in_mean, const float* in_invstd, const float* in_gamma,
                                const float* in_beta, void* ws, size_t ws_bytes, void* stream);
int mla_conv2d_dgrad_split_bnmask(const float* dy, const void* wsplit, float* dx, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                  int stride, int pad, const mla_bn_reduce_req* reqs, int nreq, int* bn_tiles, const float* mask_gamma,
                                  const float* mask_beta, void* stream);
/* measurement / test hook: 0 = one launch per output parity class of a stride-2 input gradient (split arithmetic), 1 (default;
 * $MLA_DGRAD_MERGE overrides) = all classes in one launch, longest K first; other values: query.  Returns the setting. */
int mla_conv2d_dgrad_merge(int on);
/* measurement / test hook: 0 = every split forward / input-gradient gather-GEMM is one launch, 1 (default; $MLA_CONV_TWO_PHASE overrides) =
 * row counts between whole rounds of the 256 CUs run whole rounds of a big tile and one launch of the best tile for the remaining rows;
 * other values: query.  Results do not depend on the setting (same K order per output element). */
int mla_conv2d_two_phase(int on);
int mla_conv2d_split_terms(int terms);
/* The ResNet stem (backbone.py:79-83, 149: 7x7, stride 2, pad 3, 1 or 3 -> 64 channels) on the split arithmetic, as persistent
 * patch-loader kernels: a workgroup keeps the weights (forward: three bf16 planes) resident in LDS, loads the 37 x 37 x Cin
 * input patch of a 16 x 16 output tile once and serves all 49 taps from it.  `w` / `dw` are the plain fp32 HWIO weights (the
 * forward splits them in its prologue).  mla_conv2d_stem_supported() != 0 for the shapes these entries accept; everything else
 * (and conv_math = f32) runs on mla_conv2d_fwd / mla_conv2d_wgrad.  bn_partial as in mla_conv2d_fwd, fp64 partials, one row per
 * workgroup (>= mla_conv2d_stem_fwd_partial_elems() floats); *bn_tiles receives the row count for mla_bn_finalize. */
int mla_conv2d_stem_supported(int Cin, int Cout, int KH, int KW, int stride, int pad);
/* measurement hook: force 4 or 8 waves per stem-forward workgroup, 0 = automatic (4 for Cin = 1, 8 for Cin = 3); other values: query */
int mla_conv2d_stem_waves(int waves);
size_t mla_conv2d_stem_fwd_partial_elems(void);
int mla_conv2d_stem_fwd_split(const float* x, const float* w_hwio, float* y,
                              int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                              float* bn_partial, int* bn_tiles, void* stream);
size_t mla_conv2d_stem_wgrad_split_ws_bytes(int Cin);
int mla_conv2d_stem_wgrad_split(const float* x, const float* dy, float* dw_hwio,
                                int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                void* ws, size_t ws_bytes, void* stream);
/* mla_conv2d_stem_wgrad_split with the apply pass of the stem's BatchNorm / max-pool backward (backbone.py:149-152) formed
 * inside: instead of dy it reads conv1's output y (N,OH,OW,64), the pooled gradient dpool and window codes idx (N,PH,PW,64) and
 * bn1's vectors, and forms dy = gamma * invstd * ([bn(y) > 0] g - dbeta/M - xhat * dgamma/M) where it would have loaded it
 * (the expression of mla_bn_bwd_pooled, bit for bit: dw equals mla_bn_bwd_pooled + mla_conv2d_stem_wgrad_split).  dgamma /
 * dbeta: from mla_bn_bwd_pooled with dy = NULL.  Same workspace as mla_conv2d_stem_wgrad_split. */
int mla_conv2d_stem_wgrad_split_bnpool(const float* x, const float* dpool, const uint8_t* idx, const float* y,
                                       const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       const float* dgamma, const float* dbeta, float* dw_hwio,
                                       int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                       void* ws, size_t ws_bytes, void* stream);
/* measurement hook: force tile 0..4 (256x128, 128x128, 128x64, 64x64, 256x64) where Cout allows; -1 = automatic */
int mla_conv2d_split_cfg(int cfg);

/* ---- convolution, single-product bf16 arithmetic (conv_math "bf16") ------------------------------
 * y = sum bf16_rne(a) * bf16_rne(b), fp32 accumulate on v_mfma_f32_32x32x16_bf16: each operand rounded ONCE to bf16 and multiplied
 * once -- the hi * hi product of the split set alone.  fp32 in, fp32 out, same epilogues; NOT fp32-equivalent (relative error
 * ~2^-8 per product).  One-plane forms of the split gather-GEMM and per-tap weight-gradient kernels: a third of the LDS image, a
 * sixth of the MFMAs.  The arithmetic is selected by calling these entry points: they read none of the process-wide hooks above,
 * so callers of different arithmetic share a process.  Weights are converted by mla_conv2d_wimage_bf16 into
 * mla_conv2d_wimage_bytes_bf16 of scratch, one bf16 plane [tap][n][k]: transposed = 1 for the forward, 0 for the input gradient
 * (mla_conv2d_wimage_batch_bf16: descriptor rows as in mla_conv2d_wsplit_batch).  Cin, Cout multiples of 64.
 * mla_conv2d_dgrad_bf16: class_mask / residual_mask as in mla_conv2d_dgrad_classes, one launch per parity class.
 * mla_conv2d_tile_bf16 (diagnostic / test query, not needed to run the mode): the tile (index into 256x128, 128x128, 128x64, 64x64,
 * 256x64, 192x128) a gather-GEMM of M output rows, Cout columns and k_total = taps * Cin picks ON THE CURRENT DEVICE -- the choice
 * depends on its CU count (256 is assumed when there is no device); -1 for dims it does not take. */
size_t mla_conv2d_wimage_bytes_bf16(int Cin, int Cout, int KH, int KW);
int mla_conv2d_wimage_bf16(const float* w_hwio, void* wimage, int Cin, int Cout, int KH, int KW, int transposed, void* stream);
int mla_conv2d_wimage_batch_bf16(const float* params, void* wimage, const int* desc, int n, int total_blocks, void* stream);
int mla_conv2d_tile_bf16(int M, int Cout, int k_total);
int mla_conv2d_fwd_bf16(const float* x, const void* wimage_t, float* y,
                        int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                        float* bn_partial, int* bn_tiles, void* stream);
int mla_conv2d_dgrad_bf16(const float* dy, const void* wimage, float* dx,
                          int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          const float* residual, const float* relu_src, int class_mask, int residual_mask, void* stream);
size_t mla_conv2d_wgrad_ws_bytes_bf16(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int mla_conv2d_wgrad_bf16(const float* x, const float* dy, float* dw_hwio,
                          int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm2d, training mode (backbone.py:29, 32, 86, 128) -------------------------------- */
/* x is [M][C] (M = N*H*W).  Statistics: either mla_bn_stats (reads x) or conv-fused partials. */
size_t mla_bn_partial_scratch_elems(int C);   /* reduction scratch tail included in every *_partial_elems / *_ws_elems below */
size_t mla_bn_stats_partial_elems(int M, int C);
int mla_bn_stats_partial(const float* x, int M, int C, float* partial, int* tiles, void* stream);
/* Reduce partials in fp64 -> mean, invstd (biased var, eps), running stats (unbiased var, momentum). */
int mla_bn_finalize(const float* partial, int tiles, int M, int C, float eps, float momentum,
                    float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
/* out = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ) */
int mla_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma,
                 const float* beta, const float* residual, float* out, int M, int C, int relu, void* stream);
/* Backward.  g = dout * (relu_out > 0) if relu_out else dout;
 * dgamma = sum g*xhat, dbeta = sum g, dx = gamma*invstd*(g - dbeta/M - xhat*dgamma/M).
 * g_out (nullable) receives g (the gradient of the residual branch).  ws: mla_bn_bwd_ws_elems floats. */
size_t mla_bn_bwd_ws_elems(int M, int C);
int mla_bn_bwd(const float* dout, const float* relu_out, const float* x, const float* mean,
               const float* invstd, const float* gamma, float* dx, float* dgamma, float* dbeta,
               float* g_out, float* ws, int M, int C, void* stream);

/* BatchNorm backward whose reduction pass was done by the producer of dout (mla_conv2d_dgrad[_split]_bn): finalize the
 * `tiles` per-tile sums of `partial` into dgamma / dbeta, then dx = gamma * invstd * (dout - dbeta/M - xhat * dgamma/M). */
int mla_bn_bwd_from_partial(const float* dout, const float* x, const float* mean, const float* invstd, const float* gamma,
                            float* dx, float* dgamma, float* dbeta, float* partial, int tiles, int M, int C, void* stream);
/* Stem conv1 -> bn1 -> relu -> maxpool (backbone.py:149-152) without materialising the ReLU output: the max-pool applies
 * BN + ReLU to y (NHWC conv output) on the fly; out (N,OH,OW,C), idx = window position 0..8 of the first maximum. */
int mla_bn_relu_maxpool_fwd(const float* y, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* out, uint8_t* idx, int N, int H, int W, int C, void* stream);
/* ... and its backward: BatchNorm backward whose upstream gradient is gathered from the POOLED gradient dpool (N,OH,OW,C)
 * through idx and masked by bn(y) > 0; dy (N,H,W,C) = gradient w.r.t. y, dgamma / dbeta written; ws >= mla_bn_bwd_ws_elems(N*H*W, C):
 * the partial rows of the reduction over the N*OH*OW pooled rows are fitted into that at every admitted shape.
 * dy = NULL: the reduction half alone (dgamma, dbeta) -- for a consumer that forms dy itself
 * (mla_conv2d_stem_wgrad_split_bnpool). */
int mla_bn_bwd_pooled(const float* dpool, const uint8_t* idx, const float* y, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float* dy, float* dgamma, float* dbeta, float* ws,
                      int N, int H, int W, int C, void* stream);

/* ---- pooling ---------------------------------------------------------------------------------- */
/* nn.MaxPool2d(3,2,1) (backbone.py:88,152); idx = window position 0..8 of the first maximum. */
int mla_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
/* dx = scatter(dy) [* (relu_src > 0)] */
int mla_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, const float* relu_src, float* dx,
                         int N, int H, int W, int C, void* stream);
/* adaptive_avg_pool2d/3d(.,1)+flatten (basic_model.py:56-65): x [NB][P][C] -> y [NB][C] */
int mla_avgpool_fwd(const float* x, float* y, int NB, int P, int C, void* stream);
/* dx[nb][p][c] = dy[nb][c]/P [* (relu_src > 0)]  (relu_src: the pooled tensor, output of the last ReLU) */
int mla_avgpool_bwd(const float* dy, const float* relu_src, float* dx, int NB, int P, int C, void* stream);

/* ---- shared head + cross entropy (fusion_modules.py:19; main.py:130, 432-435, 444-447) ------- */
/* logits = X W^T + b; loss = -sum_i log softmax(logits_i)[label_i] * inv_batch (rank-local part);
 * dlogits = (softmax - onehot) * inv_batch; dW = dlogits^T X; db = sum dlogits; dX = dlogits W.
 * Two launches (wave per sample, then the BxD contraction).  X [B][D], W [C][D], labels int64 [B];
 * C <= 128.  ws: mla_head_ws_elems(B, C) floats: dlogits [B][C], then the row losses [B].
 * A label outside [0, C) yields a NaN loss and a zero dlogits row: that sample adds nothing to dW and db and its dX row is zero
 * (the policy of mla_ce_fwd_bwd, the concat head and the QMF heads; the fused call is the mla_head_logits -> mla_ce_fwd_bwd ->
 * mla_head_bwd chain bit for bit, bad labels included).  The logits do not depend on the labels.
 * Every loss of this family is formed per row as log(sum exp(l - max)) - (l[label] - max), the two terms of log_softmax. */
size_t mla_head_ws_elems(int B, int C);
int mla_head_ce_fwd_bwd(const float* X, const float* W, const float* b, const int64_t* labels,
                        float* logits, float* loss, float* dW, float* db, float* dX, float* ws,
                        int B, int D, int C, float inv_batch, void* stream);

/* The same head where autograd splits it, for the nn.Module / autograd.Function protocol (main.py:432-435 executed
 * literally: `out = fc_out(a)`; `loss = criterion(out, label)`; `loss.backward()`):
 *   mla_ce_fwd_bwd   nn.CrossEntropyLoss() (main.py:130), mean reduction: loss and dlogits = (softmax - onehot) * inv_batch
 *                    in one pass; ws: B floats (the row losses).  A label outside [0, C) yields a NaN loss (the reference
 *                    asserts) and a zero dlogits row.  Any C.
 *   mla_head_bwd     autograd of nn.Linear (fusion_modules.py:19) for a given dlogits: dW = s dlogits^T X, db = s sum dlogits,
 *                    dX = s dlogits W  (s = 1/world under data parallel, else 1).
 *   mla_scale_by_device_scalar   x *= *scalar, the scalar read on the device (gradient flowing into a loss node). */
int mla_ce_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, float* ws,
                   int B, int C, float inv_batch, void* stream);
int mla_head_bwd(const float* X, const float* W, const float* dlogits, float* dW, float* db, float* dX,
                 int B, int D, int C, float scale, void* stream);
int mla_scale_by_device_scalar(float* x, const float* scalar, size_t n, void* stream);

/* ---- concatenated fusion head of the joint step (fusion_modules.py:16-35; main.py:164-168, 232-237, 273-311) ----------
 * ConcatFusion.fc_out = nn.Linear(M*D, C) on cat(x_0 .. x_{M-1}) without materialising the concatenation: x_m [B][D]
 * (x2 / dx2 NULL when M = 2), W [C][M*D] (the reference's row-major layout, column block m = W_m), M = 2 or 3, C <= 128.
 *   out = sum_m x_m W_m^T + b                    [B][C]    (fusion_modules.py:22-23, 32-34)
 *   out_m = x_m W_m^T + b / M                    [M][B][C] (the half / third-head logits of main.py:283-302)
 * mla_concat_head_ce_fwd_bwd: the training head of main.py:305-310 in two launches: `out`, `out_m`,
 *   loss = -sum_i log softmax(out_i)[label_i] * inv_batch (rank-local part), loss_m[M] = the same for out_m (the reported
 *   losses of main.py:307-309, never differentiated), dlogits = (softmax - onehot) * inv_batch, dW = dlogits^T cat(x)
 *   (into W's column blocks), db = sum dlogits, dx_m = dlogits W_m.  A label outside [0, C) yields NaN losses and a zero
 *   dlogits row.  ws: mla_concat_head_ws_elems(B, C, M) floats.
 * mla_concat_head_fwd: out and out_m only (valid(), main.py:539-619, 653-679; the autograd forward), one launch.
 * mla_concat_head_bwd: autograd of the concatenated Linear for a given dlogits: dW = s dlogits^T cat(x), db = s sum dlogits,
 *   dx_m = s dlogits W_m (s = 1/world under data parallel, else 1), two launches.
 * No atomics; every reduction in a fixed order (bitwise reproducible). */
size_t mla_concat_head_ws_elems(int B, int C, int M);
int mla_concat_head_ce_fwd_bwd(const float* x0, const float* x1, const float* x2, const float* W, const float* b,
                               const int64_t* labels, float* out, float* out_m, float* loss, float* loss_m, float* dW,
                               float* db, float* dx0, float* dx1, float* dx2, float* ws, int M, int B, int D, int C,
                               float inv_batch, void* stream);
int mla_concat_head_fwd(const float* x0, const float* x1, const float* x2, const float* W, const float* b, float* out,
                        float* out_m, int M, int B, int D, int C, void* stream);
int mla_concat_head_bwd(const float* x0, const float* x1, const float* x2, const float* W, const float* dlogits, float* dW,
                        float* db, float* dx0, float* dx1, float* dx2, int M, int B, int D, int C, float scale, void* stream);

/* ---- sum / FiLM / gated fusion heads of the joint step (fusion_modules.py:5-13, 38-67, 70-98; main.py:24, 273-310, 610-614) ------
 * Two features x, y [B][D]; every Linear in the reference's (out, in) row-major layout; D a multiple of 64 (at most 4096), C <= 128.
 * Anything else is MLA_ERR_INVALID_ARG before any launch.
 *   sum    out = (x Wx^T + bx) + (y Wy^T + by)  (fusion_modules.py:12);  out_a = x Wx^T + bias_scale bx, out_v = y Wy^T + bias_scale by
 *          with bias_scale 1 in training (main.py:292-295) and 0.5 in evaluation (main.py:610-614).  Wx, Wy [C][D].
 *   FiLM   h = film W^T + b [B][2D], gamma = h[:, :D], beta = h[:, D:], z = gamma * t + beta, out = z Wout^T + bout
 *          (fusion_modules.py:53-67).  W [2D][D], Wout [C][D].  The caller passes (film, t) = (x, y) under x_film, else (y, x).
 *   gated  hx = x Wx^T + bx, hy = y Wy^T + by [B][D], z = sigmoid(hx) * hy (x_gate) or hx * sigmoid(hy), out = z Wout^T + bout
 *          (fusion_modules.py:87-98).  Wx, Wy [D][D], Wout [C][D].  sigmoid(h) = 1 / (1 + exp(-h)) in fp32.
 * mla_fusion_*_ce_fwd_bwd: the training head of main.py:305-310: `out` (sum: out_a, out_v; FiLM: h, z; gated: hx, hy, z),
 *   loss = -sum_i log softmax(out_i)[label_i] * inv_batch (sum: losses[3] = {loss, the same for out_a, for out_v}: the reported losses of
 *   main.py:308-309, never differentiated), dlogits = (softmax - onehot) * inv_batch and the gradient of every parameter and of both
 *   features.  A label outside [0, C) yields a NaN loss and a zero dlogits row.  sum: 2 launches; FiLM / gated: 3.
 * mla_fusion_*_fwd: the outputs only (valid(); the autograd forward).  sum: 1 launch; FiLM / gated: 2.
 * mla_fusion_*_bwd: autograd for a given dlogits [B][C], times `scale`, from the h / hx, hy and z of the forward.
 * ws: mla_fusion_ws_elems(B, D, C) floats.  No atomics; every reduction in a fixed order (bitwise reproducible). */
size_t mla_fusion_ws_elems(int B, int D, int C);
int mla_fusion_sum_ce_fwd_bwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                              const int64_t* labels, float* out, float* out_a, float* out_v, float* losses, float* dWx, float* dbx,
                              float* dWy, float* dby, float* dX, float* dY, float* ws, int B, int D, int C, float inv_batch,
                              float bias_scale, void* stream);
int mla_fusion_sum_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by, float* out,
                       float* out_a, float* out_v, int B, int D, int C, float bias_scale, void* stream);
int mla_fusion_sum_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* dlogits, float* dWx, float* dbx,
                       float* dWy, float* dby, float* dX, float* dY, float* ws, int B, int D, int C, float scale, void* stream);
int mla_fusion_film_ce_fwd_bwd(const float* film, const float* t, const float* W, const float* b, const float* Wout, const float* bout,
                               const int64_t* labels, float* out, float* h, float* z, float* loss, float* dW, float* db, float* dWout,
                               float* dbout, float* dfilm, float* dt, float* ws, int B, int D, int C, float inv_batch, void* stream);
int mla_fusion_film_fwd(const float* film, const float* t, const float* W, const float* b, const float* Wout, const float* bout,
                        float* out, float* h, float* z, int B, int D, int C, void* stream);
int mla_fusion_film_bwd(const float* film, const float* t, const float* W, const float* Wout, const float* h, const float* z,
                        const float* dlogits, float* dW, float* db, float* dWout, float* dbout, float* dfilm, float* dt, float* ws,
                        int B, int D, int C, float scale, void* stream);
int mla_fusion_gated_ce_fwd_bwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                                const float* Wout, const float* bout, const int64_t* labels, float* out, float* hx, float* hy, float* z,
                                float* loss, float* dWx, float* dbx, float* dWy, float* dby, float* dWout, float* dbout, float* dX,
                                float* dY, float* ws, int B, int D, int C, int x_gate, float inv_batch, void* stream);
int mla_fusion_gated_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                         const float* Wout, const float* bout, float* out, float* hx, float* hy, float* z, int B, int D, int C,
                         int x_gate, void* stream);
int mla_fusion_gated_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* Wout, const float* hx,
                         const float* hy, const float* z, const float* dlogits, float* dWx, float* dbx, float* dWy, float* dby,
                         float* dWout, float* dbout, float* dX, float* dY, float* ws, int B, int D, int C, int x_gate, float scale,
                         void* stream);

/* ---- QMF joint step head (--modulation QMF; main.py:170-268, 544-586; utils/utils.py:44-95; main.py:108-125) --------------
 * One Linear head per modality (audio_fc / visual_fc / txtual_fc): x_m [B][D], W_m [C][D], b_m [C] (x2 / W2 / b2 / dW2 / db2 /
 * dx2 NULL when M = 2), M = 2 or 3, C <= 128.
 *   z_m = x_m W_m^T + b_m   [M][B][C];   E_m = logsumexp z_m;   conf = E_m / 10   [M][B];   out = sum_m conf_m z_m   [B][C]
 * mla_qmf_head_fwd_bwd: the training head in four launches.  ell [M][B] = per-sample CE of z_m.  History (fp64, [M][n_data] each):
 *   correctness[m][idx_i] += ell_m[i], confidence[m][idx_i] = conf_m[i]; of several samples with one index the LAST writes (numpy's
 *   `a[idx] += v`).  Then lo / hi = min / max of correctness[m][:], n = (correctness - lo) / (hi - lo), and with j = (i + 1) mod B:
 *   target [M][B] = sign(n_i - n_j), margin [M][B] = |n_i - n_j|, r = conf_j + margin / (target ? target : 1),
 *   rank_m = inv_batch sum_i max(0, target (conf_i - r)).
 *   losses [2M + 2] = { L, CE(z_0) .. CE(z_{M-1}), rank_0 .. rank_{M-1}, CE(out) }, L = w_cml CE(out) + sum CE(z_m) + w_crl sum rank_m
 *   ((w_cml, w_crl) = (1, 0.1): main.py:265-268; (0, 1): main.py:203, 229).  dW_m, db_m, dx_m: the gradients of L (conf detached in
 *   `out`, both operands of a ranking pair carry gradient).  A label outside [0, C) or an index outside [0, n_data): NaN losses for
 *   that sample (and the ranking pairs it is part of), no History write, zero gradient rows.
 *   ws: mla_qmf_head_ws_elems(B, C, M) floats, 8-byte aligned.
 * mla_qmf_head_fwd: z, out and conf only (valid(), main.py:576-586), one launch.
 * No atomics, one writer per History entry, every reduction in a fixed order (bitwise reproducible). */
size_t mla_qmf_head_ws_elems(int B, int C, int M);
int mla_qmf_head_fwd_bwd(const float* x0, const float* x1, const float* x2, const float* W0, const float* W1, const float* W2,
                         const float* b0, const float* b1, const float* b2, const int64_t* labels, const int64_t* idx,
                         double* correctness, double* confidence, int n_data, float* z, float* out, float* conf, float* ell,
                         float* target, float* margin, float* losses, float* dW0, float* dW1, float* dW2, float* db0, float* db1,
                         float* db2, float* dx0, float* dx1, float* dx2, float* ws, int M, int B, int D, int C, float w_cml,
                         float w_crl, float inv_batch, void* stream);
int mla_qmf_head_fwd(const float* x0, const float* x1, const float* x2, const float* W0, const float* W1, const float* W2,
                     const float* b0, const float* b1, const float* b2, float* z, float* out, float* conf, int M, int B, int D,
                     int C, void* stream);

/* ---- GSPlugin.before_update (utils/utils.py:24-41) ------------------------------------------- */
/* r[j] = scale * sum_i X[i][j]   (column mean with scale = 1/B; rank-local column sum otherwise) */
int mla_colsum(const float* X, float* r, int B, int D, float scale, void* stream);
/* k = Pl r^T; Pl <- Pl - (k k^T) ./ (alpha + k r) ; Pl <- Pl/||Pl||_F ; G <- G Pl^T.
 * Pl [D][D] and G [C][D] are updated in place.  ws: mla_gs_ws_elems(D, C) floats. */
size_t mla_gs_ws_elems(int D, int C);
int mla_gs_project(float* Pl, const float* r, float* G, int D, int C, float alpha, float* ws, void* stream);
/* gs_mode="owm": the same step with the scalar denominator of the recursive-least-squares / OWM rule the published one was taken
 * from.  Only utils/utils.py:36-40 change; the skipped first call, alpha, r = mean(X, 0), update before projection, grad <- grad Pl^T
 * and the exp_count accounting stay the reference's:
 *     k  = Pl r^T                        (D)
 *     s  = alpha + r . k                 (scalar; >= alpha when Pl is PSD)
 *     Pl <- Pl - k k^T / s               (no renormalisation)
 *     G  <- G Pl^T                       (with the updated Pl)
 * fp32 in, out and accumulate.  Every sum is taken in mla_gs_project's lane / stride order and there are no atomics: two calls on the
 * same inputs give the same bits.  The element update is Pl[i][j] - (k_i * k_j) / s, symmetric in (i, j): a Pl that starts symmetric
 * stays symmetric bit for bit.  Two launches and no copy.  Any D, C > 0 with D <= 8192 (a row of Pl is kept in LDS); ws:
 * mla_gs_owm_ws_elems(D, C) = D + C * D floats, overlapping none of Pl, r and G. */
size_t mla_gs_owm_ws_elems(int D, int C);
int mla_gs_project_owm(float* Pl, const float* r, float* G, int D, int C, float alpha, float* ws, void* stream);

/* ---- head-only modality phase on stored features (models/basic_model.py:278-319 CLIPClassifier; main.py:432-442) ----
 * One call = one phase: out = fc_out(X) (main.py:432), loss = CE(out, labels) (:434), the head gradients of loss.backward() (:435),
 * GSPlugin.before_update on the weight gradient when `project` (:437; utils/utils.py:34-41 literally, in mla_gs_project's order with
 * r, k, the denominator, the norm and the projected sums carried in fp64 and each stored value rounded once), and
 * torch.optim.SGD(momentum, weight decay) on weight and bias (:439), in place.  No dX is formed: nothing lies behind the features.
 * X (B, D), labels int64 (B); W (C, D), b (C) and buf (C*D + C: the momentum of [W | b], `first` != 0: it becomes g + wd p);
 * Pl (D, D), read and updated only when `project`; logits (B, C) and loss[1] out; ws: mla_feature_ws_elems(B, D, C) floats.
 * 4 kernel launches and no copy when projecting, 2 otherwise; no atomics, bit-reproducible.  A label outside [0, C) poisons the loss
 * with NaN and gives a zero dlogits row: that sample adds nothing to the gradient, the momentum or the update (mla_head_ce_fwd_bwd's
 * policy).  C <= 128, D <= 4096; X, W, buf, Pl, logits and ws 16-byte aligned.  Any D and C*D (nothing here needs a multiple of 4). */
size_t mla_feature_ws_elems(int B, int D, int C);
int mla_feature_phase(const float* X, const int64_t* labels, float* W, float* b, float* buf, float* Pl, float* logits,
                      float* loss, float* ws, int B, int D, int C, float inv_batch, int project, double alpha, float lr,
                      float momentum, float wd, int first, void* stream);
/* The same phase with mla_gs_project_owm's rule in place of the literal one, in fp32: same arguments, workspace and limits.  3 kernel
 * launches when projecting (r and k in the gradient launch, then s, the row update, the projection and SGD in one), 2 otherwise. */
int mla_feature_phase_owm(const float* X, const int64_t* labels, float* W, float* b, float* buf, float* Pl, float* logits,
                          float* loss, float* ws, int B, int D, int C, float inv_batch, int project, double alpha, float lr,
                          float momentum, float wd, int first, void* stream);
/* The batch feed of such a model (dataset/dataset.py:864-872 CLIPDataset.__getitem__) from device-resident tables: row idx[b] of
 * T0 and T1 (N, D) -> out0 / out1 (B, D), labels[idx[b]] -> out_label (B), idx[b] -> out_idx (B, 1), one launch; 16-byte row
 * accesses when D % 4 == 0 and the tables are 16-byte aligned, scalar otherwise.  The kernel clamps an index to [0, N) and never
 * reads out of bounds; refusing a bad index is mla_gather_index_check's part, on the host vector the index is uploaded from. */
int mla_gather_index_check(const int64_t* idx_host, int n, int N);
int mla_gather_rows2(const float* T0, const float* T1, const int64_t* labels, const int64_t* idx, float* out0, float* out1,
                     int64_t* out_label, int64_t* out_idx, int N, int D, int B, void* stream);

/* ---- OGM / OGM-GE gradient modulation (main.py:312-410, --modulation OGM | OGM_GE) ---------------------------------
 * mla_ogm_coeff: score_m = sum_i softmax(out_m)[i][label_i] (row order), ratios and the coefficient of every modality
 *   (main.py:373-384 for M = 2: {audio, visual}; 314-337 for M = 3: {audio, visual, text}) -> coeff[M] on the device;
 *   info (nullable, 6 floats): scores at [0..M), ratios at [3..3+M).
 * mla_ogm_modulate: for each segment (= one 4-D conv gradient; seg_desc int64 [n_seg][2] = {offset, numel} into `grad`,
 *   device memory): grad = grad * *coeff, and with ge != 0 additionally + N(0, std + 1e-8), std = unbiased standard
 *   deviation of the UNSCALED segment (main.py:397-400).  first_chunk (int [n_seg + 1], device): prefix sum of
 *   ceil(numel / mla_ogm_chunk_elems()) per segment; total_chunks = first_chunk[n_seg].  Noise: Philox4x32-10 keyed by
 *   `seed`, stream (step, segment), counter = element / 4 -> reproducible, independent of the launch geometry. */
int mla_ogm_coeff(const float* out0, const float* out1, const float* out2, const int64_t* labels, int M, int B, int C,
                  float alpha, float* coeff, float* info, void* stream);
int mla_ogm_chunk_elems(void);
size_t mla_ogm_ws_bytes(int total_chunks, int n_seg);
int mla_ogm_modulate(float* grad, const int64_t* seg_desc, const int* first_chunk, int n_seg, int total_chunks,
                     const float* coeff, int ge, uint64_t seed, uint64_t step, void* ws, size_t ws_bytes, void* stream);

/* ---- transformer encoders (M3AE, models/m3ae.py; CAV-MAE, models/cav_mae.py) ------------------- */
/* nn.Linear on the gather-GEMM: y[g][y_off+r][:] = x[g][x_off+r][:] . w_kn (+ bias) (+ residual);
 * rows are `groups` x `rows` tokens taken at an offset inside groups of *_group_rows tokens (no copies for
 * "tokens 1..256 of each 257-token sequence").  w_kn is [K][N] = nn.Linear.weight^T.  y_gelu (nullable)
 * additionally receives gelu(y) (erf form, F.gelu, m3ae.py:77).  K, N multiples of 64. */
int mla_linear_fwd(const float* x, const float* w_kn, const float* bias, const float* residual, float* y,
                   float* y_gelu, int groups, int rows, int x_group_rows, int x_off, int y_group_rows, int y_off,
                   int K, int N, void* stream);
/* dx = dy . w_kn^T (+ residual) (* gelu'(gelu_src)).  wt_ws: K*N floats. */
int mla_linear_dgrad(const float* dy, const float* w_kn, float* dx, const float* residual, const float* gelu_src,
                     float* wt_ws, int groups, int rows, int dy_group_rows, int dy_off, int dx_group_rows, int dx_off,
                     int K, int N, void* stream);
/* dw_kn[K][N] = sum_rows x^T dy (dy dense [groups*rows][N]); deterministic split-K like mla_conv2d_wgrad. */
size_t mla_linear_wgrad_ws_bytes(int M, int K, int N);
int mla_linear_wgrad(const float* x, const float* dy, float* dw_kn, int groups, int rows, int x_group_rows, int x_off,
                     int K, int N, void* ws, size_t ws_bytes, void* stream);
/* The same three on the split-bf16 arithmetic (see mla_conv2d_*_split): weights pre-split with
 * mla_conv2d_wsplit(w_kn, out, Cin = K, Cout = N, 1, 1, transposed, stream), transposed = 1 for the forward image
 * (wsplit_t), 0 for the input-gradient image (wsplit). */
int mla_linear_fwd_split(const float* x, const void* wsplit_t, const float* bias, const float* residual, float* y,
                         float* y_gelu, int groups, int rows, int x_group_rows, int x_off, int y_group_rows, int y_off,
                         int K, int N, void* stream);
int mla_linear_dgrad_split(const float* dy, const void* wsplit, float* dx, const float* residual, const float* gelu_src,
                           int groups, int rows, int dy_group_rows, int dy_off, int dx_group_rows, int dx_off,
                           int K, int N, void* stream);
size_t mla_linear_wgrad_split_ws_bytes(int M, int K, int N);
int mla_linear_wgrad_split(const float* x, const float* dy, float* dw_kn, int groups, int rows, int x_group_rows, int x_off,
                           int K, int N, void* ws, size_t ws_bytes, void* stream);
/* ... and the bias gradient dbias[N] = column sums of dy out of the same pass (dbias may be NULL); workspace as reported by
 * mla_linear_wgrad_split_ws_bytes (weight slabs + one bias row per split-K range). */
int mla_linear_wgrad_split_bias(const float* x, const float* dy, float* dw_kn, float* dbias, int groups, int rows,
                                int x_group_rows, int x_off, int K, int N, void* ws, size_t ws_bytes, void* stream);
/* The same on the single-product bf16 arithmetic (see mla_conv2d_*_bf16): weights converted with
 * mla_conv2d_wimage_bf16(w_kn, out, Cin = K, Cout = N, 1, 1, transposed, stream). */
int mla_linear_fwd_bf16(const float* x, const void* wimage_t, const float* bias, const float* residual, float* y,
                        float* y_gelu, int groups, int rows, int x_group_rows, int x_off, int y_group_rows, int y_off,
                        int K, int N, void* stream);
int mla_linear_dgrad_bf16(const float* dy, const void* wimage, float* dx, const float* residual, const float* gelu_src,
                          int groups, int rows, int dy_group_rows, int dy_off, int dx_group_rows, int dx_off, int K, int N,
                          void* stream);
size_t mla_linear_wgrad_ws_bytes_bf16(int M, int K, int N);
int mla_linear_wgrad_bf16(const float* x, const float* dy, float* dw_kn, int groups, int rows, int x_group_rows, int x_off,
                          int K, int N, void* ws, size_t ws_bytes, void* stream);
int mla_linear_wgrad_bias_bf16(const float* x, const float* dy, float* dw_kn, float* dbias, int groups, int rows,
                               int x_group_rows, int x_off, int K, int N, void* ws, size_t ws_bytes, void* stream);
/* out[c] = sum_rows x[r][c]  (bias gradients).  ws: mla_colreduce_ws_elems(M, C) floats; C % 64 == 0. */
size_t mla_colreduce_ws_elems(int M, int C);
int mla_colsum_rows(const float* x, float* out, float* ws, int M, int C, void* stream);
/* nn.LayerNorm (m3ae.py:138,142,176) over rows of D (512/768/1024); saves mean and rstd per row. */
int mla_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd,
                      int M, int D, float eps, void* stream);
/* dx = LN'(dy) (+ add), dw = sum dy*xhat, db = sum dy.  dx may alias dy or add.  ws: mla_colreduce_ws_elems. */
int mla_layernorm_bwd(const float* dy, const float* x, const float* w, const float* mean, const float* rstd,
                      const float* add, float* dx, float* dw, float* db, float* ws, int M, int D, void* stream);
/* Strided batched GEMM for attention (m3ae.py:109, 121): C[z] = alpha * A[z] . B[z], z = (batch, head);
 * strides in elements (>= 0): a = {batch, head, row i, k}, b = {batch, head, k, col j}, c = {batch, head, i, j}.
 * *_extent: elements addressable from each pointer; a descriptor that reaches beyond them returns MLA_ERR_INVALID_ARG
 * (the materialised attention path; the encoders use mla_attention_* by default). */
int mla_bgemm(const float* A, const float* B, float* C, int batches, int heads, int M, int N, int K,
              const long* a_strides, const long* b_strides, const long* c_strides,
              size_t a_extent, size_t b_extent, size_t c_extent, float alpha, void* stream);
/* In-place softmax over the last axis of S (B,H,n,n); pad_mask (B,n) float, > 0 -> score := -1e7 (m3ae.py:111-118). */
int mla_softmax_fwd(float* S, const float* pad_mask, int B, int H, int n, void* stream);
/* dS = P * (dP - rowsum(dP*P)), in place in dP. */
int mla_softmax_bwd(const float* P, float* dP, int B, int H, int n, void* stream);

/* Fused multi-head attention (models/m3ae.py:102-125; timm Attention behind cav_mae.py:93), exact fp32 MFMA, head dim 64.
 * qkv (B, n, 3, H, 64) as written by the fused qkv Linear; pad_mask (B, n) float or null (mask > 0: score := -1e7,
 * m3ae.py:111-117); o (B, n, H*64); lse (B, H, n) = log-sum-exp of every score row (saved for the backward).  The n x n
 * scores never reach HBM: online softmax forward, recomputation backward (two kernels: dQ owns query rows and also writes
 * dvec (B, H, n) = rowsum(d_o * o); dK / dV own key rows), no atomics -> bitwise reproducible.  dqkv has qkv's layout. */
int mla_attention_fwd(const float* qkv, const float* pad_mask, float* o, float* lse, int B, int H, int n, int hd, void* stream);
int mla_attention_bwd(const float* d_o, const float* qkv, const float* o, const float* lse, const float* pad_mask,
                      float* dqkv, float* dvec, int B, int H, int n, int hd, void* stream);
/* The same attention (models/m3ae.py:102-125; cav_mae.py:93) on the split-bf16 arithmetic: fp32 in, out and accumulate, the five
 * products (S = Q K^T, O = P V, dP = dO V^T, dQ = dS K, dK = dS^T Q, dV = P^T dO) from the exact three-way bf16 split of both
 * operands, six kept products on the 32x32x16 bf16 MFMA (the arithmetic of mla_conv2d_*_split and the split Linear).  Arguments,
 * layouts, the rejections (hd != 64, n <= 0, B * n * 3 * H * hd >= 2^31: MLA_ERR_INVALID_ARG before any launch), the mask rule
 * and the bitwise reproducibility are mla_attention_fwd / _bwd's; n <= 3 runs their vector kernels.  Same accuracy against fp64
 * (profiles/attention_split_score_range.json).  Time of forward + backward relative to mla_attention_fwd / _bwd, same process, three
 * runs each, B = 64, H = 12 (larger (max - min) / median of the two in brackets; profiles/r07_attention_math.txt):
 * faster at tile-aligned lengths -- n = 256: 0.70 masked [0.017], 0.72 [0.016]; 288: 0.70 [0.006]; 512 (B = 32): 0.68 [0.037] --, level
 * at n = 257 (0.955 masked [0.073], 0.950 [0.005]), slower with two or three remainder rows (n = 258: 1.16 [0.002]). */
int mla_attention_fwd_split(const float* qkv, const float* pad_mask, float* o, float* lse, int B, int H, int n, int hd, void* stream);
int mla_attention_bwd_split(const float* d_o, const float* qkv, const float* o, const float* lse, const float* pad_mask,
                            float* dqkv, float* dvec, int B, int H, int n, int hd, void* stream);
/* forward_representation token assembly (m3ae.py:342-366): x0[b][0] = cls; x0[b][1+i] = (table[ids[b][i]] if
 * table else x0[b][1+i]) + pos[i] + type.  x0 is (B, L+1, D).  cls == NULL (CAV-MAE, cav_mae.py:341-343): no
 * [cls] row, x0 is (B, L, D) and x0[b][i] += pos[i] + type.  V = rows of `table`; a token id outside [0, V) makes its row
 * NaN (nn.Embedding asserts there) and receives no gradient. */
int mla_tokens_assemble(float* x0, const float* table, const int64_t* ids, const float* pos, const float* type,
                        const float* cls, int B, int L, int D, int V, void* stream);
/* its gradients: dcls, dtype (needs colsum_all = column sum of dx0 over all B*(L+1) rows) and, for text,
 * dtable[ids] += dx0 rows (nn.Embedding backward, m3ae.py:306, 360; dtable pre-zeroed by the caller).  Deterministic since
 * ABI 3: ids are sorted on the device and the rows of one id are added in ascending token order (no float atomics), so
 * repeated runs agree bit for bit.  ws >= mla_tokens_assemble_bwd_ws_bytes (only read when dtable != NULL). */
size_t mla_tokens_assemble_bwd_ws_bytes(int B, int L, int D);
int mla_tokens_assemble_bwd(const float* dx0, const float* colsum_all, const int64_t* ids, float* dcls, float* dtype,
                            float* dtable, int B, int L, int D, int V, void* ws, size_t ws_bytes, void* stream);
/* einops 'b c (h p1) (w p2) -> b (h w) (c p1 p2)' (basic_model.py:184-186); also the im2col of CAV-MAE's
 * conv16x16/16 PatchEmbed (cav_mae.py:69-84).  transposed != 0: img is stored (B,C,W,H) (spectrogram (B,time,freq)
 * viewed as (B,1,freq,time), cav_mae.py:339-340). */
int mla_patchify(const float* img, float* out, int B, int C, int H, int W, int P, int transposed, void* stream);

/* ---- CREMA-D frame augmentation (dataset/dataset.py:128-140, 144-153) ------------------------------------------
 * N decoded RGB frames (uint8 HWC, as np.asarray(PIL.Image.convert('RGB'))), packed at arbitrary byte offsets of
 * `frames` and of any sizes, -> out fp32 (B, 3, T, out_h, out_w); frame n is sample n / T, time slot n % T (the
 * reference's image.unsqueeze(1) + cat(dim=1)).  desc int64 (N, 8) per frame: byte offset, H, W, crop top, crop left,
 * crop h, crop w, flip.  Per frame the result is bit-identical to
 *     PIL img.crop((left, top, left + w, top + h)).resize((out_w, out_h), BILINEAR)     RandomResizedCrop / Resize
 *     .transpose(FLIP_LEFT_RIGHT) if flip                                              RandomHorizontalFlip
 *     lut[c][u8]                                                                       ToTensor + Normalize
 * (Pillow's separable 8-bit resample, 22-bit fixed-point coefficients; the filter clamps to the crop, not the frame).
 * lut fp32 (3, 256) on the device.  `desc` (device, read by the kernel) and `desc_host` (host memory, the same values)
 * are both needed: the host copy is validated and planned before the launch.
 * mla_frames_check runs those host checks alone (no GPU): crop inside the frame, sizes > 0, offset + H*W*3 within
 * frames_bytes, N == B*T, and an LDS plan that fits (extreme downscales of a huge crop do not). */
int mla_frames_check(const int64_t* desc_host, int N, int B, int T, size_t frames_bytes, int out_h, int out_w);
int mla_frames_resample(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                        const float* lut, float* out, int N, int B, int T, int out_h, int out_w, void* stream);

/* ---- CAV-MAE / M3AE-eval image transform (dataset/dataset.py:251-256, 413-420) -----------------------------------
 * mla_frames_resample generalised.  desc int64 (N, 12) per frame: byte offset, H, W, crop top, crop left, crop h, crop w,
 * flip, full_h, full_w, win_top, win_left.  The crop is resized to full_h x full_w with `filter` (0 = bilinear, 1 = Pillow's
 * bicubic: a = -0.5, support 2, negative coefficients rounded away from zero) and the window
 * [win_top, win_top + out_h) x [win_left, win_left + out_w) of that image goes through the flip and the LUT into
 * out fp32 (B, 3, T, out_h, out_w).  Only the window is computed.  Per frame the result is bit-identical to
 *     PIL img.crop(box).resize((full_w, full_h), BICUBIC | BILINEAR)
 *        .crop((win_left, win_top, win_left + out_w, win_top + out_h))      Resize(size) + CenterCrop(size)
 *        .transpose(FLIP_LEFT_RIGHT) if flip;  lut[c][u8]                   ToTensor + Normalize
 * mla_image_check runs the host checks alone (no GPU): those of mla_frames_check, plus full sizes > 0, a window inside
 * the resized image and a known filter. */
int mla_image_check(const int64_t* desc_host, int N, int B, int T, size_t frames_bytes, int out_h, int out_w, int filter);
int mla_image_resample(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                       const float* lut, float* out, int N, int B, int T, int out_h, int out_w, int filter, void* stream);

/* ---- M3AE / Food-101 train image transform (dataset/dataset.py:401-412: timm create_transform, color_jitter=True) ----
 * RandomResizedCropAndInterpolation(BICUBIC) -> RandomHorizontalFlip -> torchvision ColorJitter(1, 1, 1) -> ToTensor +
 * Normalize of N images -> out fp32 (N, 3, 1, out_h, out_w).  frames / desc / lut as for mla_image_resample (filter = bicubic,
 * T = 1).  jit int64 (N, 7) per image: n_ops, op0, op1, op2, brightness bits, contrast bits, saturation bits.  The first
 * n_ops (0..3) operation ids (0 = brightness, 1 = contrast, 2 = saturation, each at most once; further slots are ignored) are
 * applied in that order to the flipped uint8 image, each as Pillow's ImageEnhance = Image.blend(degenerate, image, a):
 *     per byte, fp32, product and sum rounded separately:  t = (float)d + a * (float)(x - d);
 *     result = (uint8)t for 0 <= a <= 1, else 0 if t <= 0, 255 if t >= 255, (uint8)t otherwise
 *     d = 0 (brightness);  d = L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of the pixel (saturation);
 *     d = m = int(S / n + 0.5), S = the sum of L over the image AS IT IS WHEN CONTRAST IS APPLIED, n = out_h * out_w (contrast)
 * with a the fp32 whose bit pattern the table holds (finite, >= 0).  Per image the result is bit-identical to PIL crop ->
 * resize(BICUBIC) -> transpose -> ImageEnhance.Brightness / Contrast / Color in the given order -> lut.
 * Two launches.  staging (uint8, >= N*out_h*out_w*3 bytes) receives the image before contrast; partials (int64, 8-byte aligned,
 * >= N * ceil(out_h / band) slots, band = 16 unless the LDS plan halves it as mla_image_check describes; N * out_h always
 * suffices) the per-band luma sums.  Integer sums only: the result does not depend on the order workgroups run in.
 * `jit` (device) and `jit_host` (host, the same values) as for desc.  mla_image_augment_check runs the host checks alone (no
 * GPU): those of mla_image_check, operation ids in range and not repeated, factors finite and >= 0, staging and partials
 * large enough; mla_image_augment also refuses out, staging and partials that overlap. */
int mla_image_augment_check(const int64_t* desc_host, const int64_t* jit_host, int N, size_t frames_bytes, int out_h, int out_w,
                            size_t staging_bytes, size_t partials_count);
int mla_image_augment(const uint8_t* frames, size_t frames_bytes, const int64_t* desc, const int64_t* desc_host,
                      const int64_t* jit, const int64_t* jit_host, const float* lut, float* out, uint8_t* staging,
                      size_t staging_bytes, int64_t* partials, size_t partials_count, int N, int out_h, int out_w, void* stream);

/* ---- CAV-MAE spectrogram augmentation (dataset/dataset.py:281-294, 303-321; --cav_augnois) ----------------------
 * x, out fp32 (B, T, F), distinct buffers.  desc int64 (B, 8) per sample: flags, f0, fw, t0, tw, roll, scale_bits,
 * stream_id; flags bit 0 = masks + noise + roll on (0: the sample is only normalised); scale_bits = the fp32 bit pattern
 * of the noise scale s.  Per element, in fp32 with IEEE division and no contraction:
 *     v = (aug && (f0 <= f < f0+fw || t0 <= t < t0+tw)) ? 0 : x[b,t,f];   v = (v - mean) / std;
 *     if aug: v += (u(b, t*F + f) * s) / 10;                              out[b, (t + roll) mod T, f] = v
 * u(b, i) = (r >> 8) * 2^-24 in [0, 1) with r = word i % 4 of Philox4x32-10(counter i / 4, stream_id[b], seed).
 * This equals torch's CPU result of the reference's expressions bit for bit given the same uniforms.
 * F is a multiple of 4 and x / out are 16-byte aligned (a thread moves 4 bins: one Philox block, one 16-byte access).
 * mla_fbank_check runs the descriptor checks alone (no GPU): f0 + fw <= F, t0 + tw <= T, widths >= 0, |roll| <= T,
 * F % 4 == 0; mla_fbank_augment also refuses std == 0, misaligned and overlapping buffers. */
int mla_fbank_check(const int64_t* desc_host, int B, int T, int F);
int mla_fbank_augment(const float* x, float* out, const int64_t* desc, const int64_t* desc_host, int B, int T, int F,
                      float mean, float std, uint64_t seed, void* stream);

/* ---- Modal3Dataset missing-modality masks (dataset/dataset.py:794-801; IEMOCAP, --modal3) -----------------------
 * The reference multiplies a sample's spectrogram, image, token ids and padding mask by its 0/1 mask entries.  Here the P
 * images a batch does have are transformed into image_compact fp32 (P, 3, S, S) (P >= 0; may be NULL when P = 0) and one
 * launch finishes the batch.  mdesc int64 (B, 4) per sample: audio present, image present, text present, image slot (in
 * [0, P) when the image is present, -1 when not).
 *     image_out[b] (fp32 (B, 3, S, S)) = image_compact[slot] when the image is present, else zeros;
 *     spec[b] (fp32 (B, T*F)), token[b] (int64 (B, L)), pm[b] (fp32 (B, L)): overwritten with zeros IN PLACE when their
 *     modality is absent, otherwise not touched.
 * Selection, not multiplication: an absent row may hold NaN, Inf or garbage (the batcher does not load it) and comes out as
 * zeros with every bit clear -- +0.0 where the reference's x * 0 gives -0.0 for negative x; the values are equal.
 * 3*S*S, T*F and L are multiples of 4 and all five buffers 16-byte aligned (rows move as 16-byte units); image_out overlaps
 * no input.  `mdesc` (device) and `mdesc_host` (host, the same values) as for the other feed kernels: flags must be 0 or 1,
 * the slots of the rows with an image a permutation of 0..P-1, and P the number of such rows.
 * mla_modal3_assemble_check runs the size and table checks alone (no GPU). */
int mla_modal3_assemble_check(const int64_t* mdesc_host, int B, int P, int S, int TF, int L);
int mla_modal3_assemble(const float* image_compact, float* spec, int64_t* token, float* pm, const int64_t* mdesc,
                        const int64_t* mdesc_host, float* image_out, int B, int P, int S, int TF, int L, void* stream);

/* ---- Kaldi log-mel filterbank from PCM16 clips (data/extract_fbank.py:8-54) -------------------------------------
 * For each of B packed mono 16 kHz clips: waveform = s / 32768 - mean, then torchaudio 0.8.1's
 *     kaldi.fbank(waveform, htk_compat=True, sample_frequency=16000, use_energy=False, window_type='hanning',
 *                 num_mel_bins=128, dither=0.0, frame_shift=10)
 * (400-sample frames every 160 with snip_edges, per-frame DC removal, pre-emphasis 0.97, symmetric Hann window, 512-point
 * power spectrum, 128 mel banks over the bins 0..255, log(max(E, 2^-23))), padded with +0.0 or cut to target_length rows.
 *     wav        int16, wav_samples of them; a clip may start at any sample (2-byte alignment)
 *     desc       int64 (B, 4) per clip: offset_samples, n_samples, sample_sum, reserved (0).  n_samples is 0 (an absent clip:
 *                all rows +0.0) or >= 400; sample_sum is the exact integer sum of the clip's samples, from which the clip mean
 *                is float(double(sample_sum) / (32768.0 * n_samples))
 *     window     fp32 (400); twiddle fp32 (512, 2): (cos, -sin)(2 pi j / 512), computed in fp64 and rounded once
 *     mel_start, mel_len int32 (128), mel_weight fp32 (mel_weights): bank i weighs the bins [mel_start[i], mel_start[i] +
 *                mel_len[i]) with the next mel_len[i] entries of mel_weight; the runs lie inside [0, 256)
 *     out        fp32 (B, target_length, 128), 16-byte aligned; every element is written
 * `desc`, `mel_start`, `mel_len` (device) and their `_host` twins (host, the same values) as for the other feed kernels.
 * A clip's rows depend on that clip alone (not on B, its neighbours or its offset) and are the same bits in every run: fixed
 * reduction orders, no atomics.  mla_wav_fbank_check runs the size and table checks alone (no GPU). */
int mla_wav_fbank_check(const int64_t* desc_host, int B, size_t wav_samples, int target_length, const int32_t* mel_start_host,
                        const int32_t* mel_len_host, size_t mel_weights);
int mla_wav_fbank(const int16_t* wav, size_t wav_samples, const int64_t* desc, const int64_t* desc_host, const float* window,
                  const float* twiddle, const int32_t* mel_start, const int32_t* mel_len, const int32_t* mel_start_host,
                  const int32_t* mel_len_host, const float* mel_weight, size_t mel_weights, float* out, int B, int target_length,
                  void* stream);

/* ---- HBM-resident CREMA-D feed (dataset/dataset.py:111-161 from device memory) ---------------------------------
 * The decoded dataset stays on the device: `frames` (uint8 HWC frames at the byte offsets of `table`), `table` int64 (N*T, 3) rows
 * (byte offset, H, W) of frame t of sample i at row i*T + t, `spec_table` fp32 (N, 1024*128) or NULL, `labels` int64 (N), and the
 * epoch's visiting `order` int64 (N).  mla_resident_batch makes batch slots j = 0..b-1 from the samples i = order[pos + j] with three
 * launches and nothing else -- no allocation, no synchronisation, no host read of device memory:
 *   draw      desc_out int64 (b*T, 8): one mla_frames_resample descriptor row per frame, label_out[j] = labels[i], idx_out[j] = i.
 *             train == 0: (offset, H, W, 0, 0, H, W, 0).  train != 0: torchvision RandomResizedCrop(scale (0.08, 1), ratio
 *             (3/4, 4/3)).get_params with its central-crop fallback, and RandomHorizontalFlip, on Philox4x32-10 in fp64:
 *               block(k) = philox4x32(counter = (t << 4) | k, stream_id = i, key = (epoch << 32) | seed), words a, b, c, d
 *               try k = 0..9:  target_area = H*W*(0.08 + 0.92*a*2^-32);  aspect = exp(L0 + (L1 - L0)*b*2^-32), L0 = log(3/4),
 *                              L1 = log(4/3);  w = rint(sqrt(target_area*aspect)), h = rint(sqrt(target_area/aspect));
 *                              accepted when 0 < w <= W and 0 < h <= H: top = (c*(H-h+1)) >> 32, left = (d*(W-w+1)) >> 32
 *               flip = word a of block(10) < 2^31
 *             so a frame's row depends on (seed, epoch, i, t) and its size alone; seed, epoch < 2^32.
 *   resample  image_out fp32 (b, 3, T, out_h, out_w): mla_frames_resample's kernel body over desc_out, the same bits.
 *   gather    spec_out fp32 (b, 1024, 128) = the rows i of spec_table (skipped when spec_table is NULL), 16-byte accesses.
 * mla_resident_plan runs once, on the host copy of the table (no GPU): 0 < H, W <= 65536, offset >= 0 and offset + H*W*3 <=
 * frames_bytes in 64-bit arithmetic, rows = N*T; then plan5 = (band, rows_cap, kh, kv, lds), the resample kernel's LDS plan maximised
 * over every crop the draw can make (every height 1..H and width 1..W of every frame shape; train == 0: the whole frames only).
 * A dataset for which no band fits 64 KB of LDS is refused with the frame size named.  A plan made with train != 0 also serves
 * train == 0.  A larger plan than a batch needs changes no bit of the result.
 * mla_resident_batch refuses on the host: pos + b > N, b*T >= 65536, seed or epoch >= 2^32, null or misaligned buffers (the int64
 * buffers 8-byte, lut / image_out 4-byte, spec_table / spec_out 16-byte), and a plan5 that is not of mla_resident_plan's making for
 * out_h, out_w (band a power of two <= 16, odd filter sizes >= 3, lds recomputed from the rest and <= 64 KB).  The order vector
 * is validated where it is made, with mla_gather_index_check; on the device an entry is clamped to [0, N) and a table row that
 * leaves the buffer becomes the 1x1 frame at offset 0, so no kernel reads out of bounds. */
int mla_resident_plan(const int64_t* table_host, int64_t rows, int T, size_t frames_bytes, int out_h, int out_w, int train,
                      int* plan5);
int mla_resident_batch(const uint8_t* frames, size_t frames_bytes, const int64_t* table, const float* spec_table,
                       const int64_t* labels, const int64_t* order, int N, int T, int pos, int b, uint64_t seed, uint64_t epoch,
                       int train, const int* plan5, const float* lut, int64_t* desc_out, float* image_out, float* spec_out,
                       int64_t* label_out, int64_t* idx_out, int out_h, int out_w, void* stream);

/* ---- rows of a batch: gather, expand, compact-and-sum (Modal3Classifier(..., present=)) ------------------------
 * A transformer encoder treats every sample on its own, so the samples of a batch whose modality is absent (all-zero input) share
 * one feature f(0), and their feature gradients reach the parameters only through their sum.  These three move the rows:
 *   mla_rows_gather       dst[j] = src[idx[j]] for j < P, then zero_tail_rows rows with every bit clear (+0.0 / token id 0).  src has
 *                         B rows of row_elems elements of elem_bytes (4 or 8) bytes; dst has P + zero_tail_rows >= 1 rows.
 *   mla_rows_expand       dst[b] = src[map[b]] for b < B: `map` int64 (B) names, for every destination row, its source row among the
 *                         src_rows rows of src (a present sample's compact row, or the row that holds f(0)); elements as for
 *                         mla_rows_gather.  The caller builds the
 *                         map on the host, so every destination row is written exactly once: no fill pass, no overwrite.
 *   mla_rows_compact_sum  dst[j] = src[idx[j]] for j < P; dst[P] = src[absent_idx[0]] + src[absent_idx[1]] + ... (A terms) in fp32,
 *                         added in that order starting from +0.0 (A == 0: +0.0).  src has B rows, dst P + 1.
 * Copies move bits (NaN payloads and -0.0 survive).  16-byte accesses when src, dst and the row size are multiples of 16 bytes,
 * 4-byte words otherwise; fixed order, no atomics, the same bits in every run.
 * Every index table comes twice, as mla_modal3_assemble's does: on the device (int64, 8-byte aligned) and the same entries on the
 * host.  The host copy is checked before anything is launched -- every entry inside [0, B) resp. [0, src_rows) -- together with:
 * null pointers, B <= 0, P outside [0, B], A < 0, row_elems == 0, no destination row or more than 65535, src / dst off a 4-byte
 * boundary, dst overlapping src: MLA_ERR_INVALID_ARG, nothing launched.  On the device an entry outside the source is never read
 * through: its row is written as zeros (resp. skipped in the sum). */
int mla_rows_gather(const void* src, const int64_t* idx, const int64_t* idx_host, void* dst, int B, int P, size_t row_elems,
                    int elem_bytes, int zero_tail_rows, void* stream);
int mla_rows_expand(const void* src, const int64_t* map, const int64_t* map_host, void* dst, int B, int src_rows,
                    size_t row_elems, int elem_bytes, void* stream);
int mla_rows_compact_sum(const float* src, const int64_t* idx, const int64_t* idx_host, const int64_t* absent_idx,
                         const int64_t* absent_host, float* dst, int B, int P, int A, size_t row_elems, void* stream);

/* ---- evaluation path (main.py:486-679 `valid`, gs_flag branch) --------------------------------- */
/* logits = X W^T + b only (main.py:636-639) */
int mla_head_logits(const float* X, const float* W, const float* b, float* logits, int B, int D, int C, void* stream);
/* Fusion + accuracy of one batch (main.py:640-676, 65-106): weights = fixed alphas or entropy gating
 * (entropy over softmax(dim=0) = the batch axis, summed over the tensor: one scalar per modality per batch, Q9);
 * fused = sum_m w_m out_m; arg-max (first maximum); int32 counters accumulated in `counts`:
 * [0,C) samples per class, [C,2C) fused-correct per class, [C(2+m), C(3+m)) modality-m-correct per class.
 * weights_out (nullable, M floats) receives the weights used.  M = 2 or 3. */
int mla_eval_fuse(const float* out0, const float* out1, const float* out2, const int64_t* labels, int* counts,
                  float* weights_out, int M, int B, int C, int dynamic, float alpha0, float alpha1, float alpha2,
                  void* stream);
/* Head + fusion + accuracy of one batch in ONE launch, with the gating taken per SAMPLE (main.py:65-106, 636-676: the rule of
 * main.py:65-87 applied to each row's own class distribution, the reference's commented-out softmax(dim=1)).  Opt-in: the
 * published batch-axis form stays mla_eval_fuse.  Per row r:
 *   l_m    = x_m W^T + b, the sum and the order of mla_head_logits: logits_out[m] (M, B, C) equals it bit for bit
 *   mode 1   H_m = - sum_c p_c lp_c with p = softmax(l_m), lp = log_softmax(l_m); a class whose exp underflows to 0 contributes
 *            0, its limit.  g_m = exp(max_k H_k - H_m), w_m = g_m / sum_k g_k over the ELIGIBLE modalities
 *   mode 0   w_m = alpha_m
 *   present  (nullable, uint8 (B, M); null = all present): a modality with present[r][m] == 0 is not eligible and gets weight
 *            +0.0; mode 1 gates over the others, mode 0 gives them alpha_m / (sum of the eligible alphas) -- a row that has every
 *            modality keeps alpha_m as it is.  The absent modality's own logits, arg-max and counter are still produced.
 *   fused  = sum_m w_m l_m (modalities in order); arg-max = first maximum, for the fused row and for each modality
 *   counts   int32, accumulated, the layout of mla_eval_fuse: [0,C) samples per class, [C,2C) fused-correct, [C(2+m), C(3+m))
 *            modality-m-correct.  Integer atomics only; every float is a function of its row alone (the same bits in every run
 *            and at every batch size).
 * fused_out (B, C), weights_out (B, M) and pred_out (B, 1 + M) int32 (fused arg-max, then each modality's) may be null.
 * A row whose label lies outside [0, C), that has no present modality, or (mode 0) whose eligible alphas do not sum to more than
 * 0 is counted nowhere: its weights_out and fused_out rows are NaN and its pred_out row is -1; every other row is intact.
 * Non-finite logits are outside the contract (nothing is indexed with them).
 * MLA_ERR_INVALID_ARG, nothing launched: M not 2 or 3; a null required pointer (x2 is required when M == 3); B, D, C <= 0;
 * C > 128 (the two-slot softmax); mode not 0 or 1; a float / int32 buffer off a 4-byte or labels off an 8-byte boundary. */
int mla_eval_head(const float* x0, const float* x1, const float* x2, const float* W, const float* b, const int64_t* labels,
                  const uint8_t* present, int* counts, float* logits_out, float* fused_out, float* weights_out, int* pred_out,
                  int M, int B, int D, int C, int mode, float alpha0, float alpha1, float alpha2, void* stream);
/* ---- evaluation metrics beyond accuracy: score store, average precision, confusion counts ---------------------------
 * valid() forms prediction = softmax(out), pred_a, pred_v (main.py:653-657) and keeps only their arg-max; the store keeps them.
 * A store of `cap` rows and H = 1 + M heads (fused first, then each modality; 1 <= H <= 4, C <= 128) is three caller-owned buffers:
 *   scores  fp32 (H, C, cap), CLASS-major: scores[h][c][n] = softmax(logits_h[n])[c] = e / s of the two-slot softmax every head uses
 *   pred    int32 (H, cap): arg-max of the LOGITS, first maximum (the evaluators' rule; not the arg-max of the rounded probabilities)
 *   labels  int32 (cap): the label as given (a value outside int32 is stored as -1)
 * The row count lives with the caller: no device counter, no synchronisation.
 *
 * mla_scores_append writes rows pos .. pos + B - 1 from the H logit matrices (B, C) of one batch and its int64 labels, in one launch.
 * weights (nullable): H - 1 floats on the device -- what mla_eval_fuse has just written, or the fixed alphas.  Then l0 must be null
 * and head 0 is formed as sum_m weights[m] l_{1+m}, modalities in order from +0.0: the expression and the order of mla_eval_fuse,
 * whose fused logits are never materialised, so the stored pred[0] is its fused arg-max.
 * MLA_ERR_INVALID_ARG, nothing launched, the store untouched: H outside [1, 4]; C <= 0 or C > 128; B <= 0; cap <= 0 or cap > 2^26;
 * pos < 0 or pos + B > cap; a null pointer among labels, the three buffers and the matrices the call reads; weights together with
 * l0 or with H == 1; a float / int32 buffer off a 4-byte or labels off an 8-byte boundary.
 *
 * mla_average_precision: ap[h][c] (fp64 (H, C)) and npos[c] (int32 (C)) over the first N rows, in two launches and without a sort.
 * For a class with P positives sklearn's average_precision_score, sum over distinct thresholds of (R_n - R_{n-1}) P_n, equals
 * (1 / P) sum over positives p of TP(>= s_p) / CNT(>= s_p): the k positives of a tie group each contribute the precision at the
 * end of their group and together its recall step k / P.  Labels are single-label, so row r owns one term, in its own class c:
 *   terms     ws[h][r] = ge ? (double)tp / (double)ge : 0.0, ge = #{n < N: scores[h][c][n] >= s}, tp = those of them with
 *             labels[n] == c, s = scores[h][c][r] (integer counts)
 *   finalize  lane l of one wave adds the ws[h][n] of its rows n = l, l + 64, ... with labels[n] == c in increasing n from +0.0, the
 *             64 lane sums are added by the xor butterfly (offsets 32, 16, .., 1), the sum is divided by npos[c]
 * That order is the definition: a restatement that follows it reproduces ap bit for bit.  ws: mla_metrics_ws_bytes(cap, H) bytes
 * (fp64 (H, cap)), holds the terms afterwards.
 * Policies: a NaN score is >= nothing and nothing is >= it, so a NaN-scored positive has ge = 0 and the term 0.0; a label outside
 * [0, C) makes its row a positive of no class and a negative of every class (term 0.0); a class with npos == 0 gets ap = NaN
 * (sklearn warns and answers 0.0 there); rows >= N of the store are never read.
 *
 * mla_confusion_count: conf[h][true][predicted] += 1 (int32 (H, C, C), accumulated: the caller zeroes it) over the first N rows,
 * integer atomics, one launch.  A row whose label lies outside [0, C) is skipped for every head, as mla_eval_fuse counts such a
 * row nowhere, not in its samples-per-class counter either; so is a prediction outside [0, C).
 * Both refuse (MLA_ERR_INVALID_ARG, nothing launched): H outside [1, 4]; C <= 0 or C > 128; cap <= 0 or cap > 2^26; N <= 0 or
 * N > cap; a null pointer; a float / int32 buffer off a 4-byte or a double buffer off an 8-byte boundary. */
int mla_scores_append(const float* l0, const float* l1, const float* l2, const float* l3, const float* weights,
                      const int64_t* labels, float* scores, int* pred, int* labels_out, int H, int B, int C, int pos, int cap,
                      void* stream);
size_t mla_metrics_ws_bytes(int cap, int H);
int mla_average_precision(const float* scores, const int* labels, int N, int cap, int H, int C, double* ap, int* npos,
                          double* ws, void* stream);
int mla_confusion_count(const int* pred, const int* labels, int N, int cap, int H, int C, int* conf, void* stream);
/* ---- fusion-weight search: the fixed-weight fusion of valid() (main.py:647-651) at every point of a grid, in ONE launch ----------
 * The per-modality logits l_m (B, C) do not depend on the fusion weights, so G candidate weightings are scored from the logits of
 * one evaluation pass.  grid: fp32 (G, M) on the device, row g = the weights of candidate g.  Tables, int32, accumulated (the caller
 * zeroes them): tp (G, C) correct per candidate and class, pp (G, C) predictions per candidate and class, num (C, nullable) samples
 * per class.  Integer atomics only, nothing synchronised; every prediction is a function of its row and its grid row alone.
 *   rows     a row whose label lies outside [0, C) or that has no present modality is counted nowhere, for any g.  Every other
 *            row adds 1 to num[label], once per row and not once per grid point.
 *   present  (nullable, uint8 (B, M); null = all present), the fixed-alpha rule of mla_eval_head (mode 0) with alpha = grid[g]:
 *            a row that has every modality uses w_m = grid[g][m] as it is; otherwise s = the eligible grid[g][m] added in order
 *            from +0.0 and w_m = eligible ? grid[g][m] / s : +0.0.  If !(s > 0) the pair (row, g) adds nothing to tp or pp; the
 *            row stays in num, so it is an error of candidate g.
 *   fused  = sum_m w_m l_m[c], modalities in order from +0.0: the expression and the order of mla_eval_fuse and mla_eval_head,
 *            contracted to fused multiply-adds as theirs is.  prediction = the first maximum (v > best from -inf, arg = 0).
 *            pp[g][prediction] += 1; tp[g][label] += 1 when they agree.
 * Nothing is indexed with a float: non-finite weights or logits are outside the contract, the prediction stays inside [0, C).
 * MLA_ERR_INVALID_ARG, nothing launched: M not 2 or 3; a null required pointer (l2 is required when M == 3; present and num may
 * be null); B, C, G <= 0; C > 128; G > 4096; a float / int32 buffer off a 4-byte or labels off an 8-byte boundary. */
int mla_fusion_sweep(const float* l0, const float* l1, const float* l2, const int64_t* labels, const uint8_t* present,
                     const float* grid, int* tp, int* pp, int* num, int M, int B, int C, int G, void* stream);
/* ---- gate search: the gated fusion family w_m ~ a_m exp(-beta H_m), a gate = (a_0 .. a_{M-1}, beta) ------------------------------
 * a: a non-negative prior per modality; beta: an inverse temperature on the per-sample entropies.  beta = 0 is the (normalised)
 * fixed-weight fusion, a = 1 and beta = 1 the gating of mla_eval_head mode 1.  The rule, per batch row, E the eligible modalities
 * (present, or all):
 *   H_k    the entropy exactly as mla_eval_head forms it in mode 1: the two-slot softmax of the row (maximum, e = expf(l - mx),
 *          s = the wave sum of e, logs = logf(s)), t = e != 0 ? (e / s) * ((l - mx) - logs) : 0 per slot, H = 0 - wave_sum(t0 + t1)
 *   hmax = max_{k in E} H_k (fmaxf from -inf, k ascending)
 * and for a gate (a, beta):
 *   x_k  = beta * (hmax - H_k)                          fp32
 *   g_k  = k in E ? a_k * expf(x_k) : +0.0              fp32
 *   sum  = sum_k (double) g_k, k = 0, 1, 2 in that order
 *   s    = (float) sum
 *   the (row, gate) pair is left out unless s > 0
 *   w_k  = k in E ? g_k / s : +0.0
 *   fused = sum_m w_m l_m[c], modalities in order from +0.0, the expression of mla_eval_fuse / mla_eval_head / mla_fusion_sweep
 *   prediction = the first maximum
 * Two identities hold bit for bit: a = 1, beta = 1 gives the weights of mla_eval_head mode 1 (both multiplications by 1 are exact);
 * beta = 0 with (float) sum_k (double) a_k == 1.0f over E gives w_k = a_k, the weights of the fixed fusion (expf(0) = 1, a / 1 is
 * exact).
 * Contract on a gate: every entry finite, 0 <= a_k <= 1024, 0 <= beta <= 16.  hmax - H_k <= ln 128, so x_k <= 16 ln 128 = 77.6 <
 * 88.7 = ln FLT_MAX, and 1024 e^77.6 = 5e36 < FLT_MAX: neither g_k nor the three-term sum can overflow.  mla_eval_head_gated checks
 * its gate; a device grid is the caller's to validate before upload: one that breaks the contract may give meaningless counts,
 * never an out-of-range index (the scan answers inside [0, C)).
 *
 * mla_gate_sweep: every gate of grid (fp32 (G, M + 1) on the device, row g = a_0 .. a_{M-1}, beta) scored on one batch's logits in
 * ONE launch.  Tables and policies are mla_fusion_sweep's: int32, accumulated; tp[g][class] and pp[g][class] per gate, num[class]
 * (nullable) once per counted row; integer atomics only.  A row whose label lies outside [0, C) or that has no present modality is
 * counted nowhere; a left-out pair adds nothing to tp / pp and its row stays in num, an error of gate g.  ent_out (nullable, fp32
 * (B, M)) receives H of every row and modality, the rows counted nowhere and the absent modalities included.
 * MLA_ERR_INVALID_ARG, nothing launched: M not 2 or 3; a null required pointer (l2 is required when M == 3; present, num and ent_out
 * may be null); B, C, G <= 0; C > 128; G > 4096; a float / int32 buffer off a 4-byte or labels off an 8-byte boundary.
 * mla_gate_sweep_tile(rows): the batch rows a workgroup stages at a time, 1 (the default), 2 or 4; any other value only queries.
 * Answers the tile in force.  The tables do not depend on it; it exists to be measured.
 *
 * mla_eval_head_gated: mla_eval_head with the gate (prior0 .. prior2, beta) in place of mode / alphas: the same arguments, outputs,
 * counter layout and bad-row policy; logits_out equals mla_head_logits bit for bit.  A pair the rule leaves out (!(s > 0)) is a bad
 * row: NaN weights_out and fused_out rows, pred_out row -1, counted nowhere.  With the same gate it predicts, on every row, what
 * that gate's row of mla_gate_sweep predicts.  Refuses what mla_eval_head refuses (there is no mode) and a gate outside the
 * contract (prior2 is not read when M == 2). */
int mla_gate_sweep(const float* l0, const float* l1, const float* l2, const int64_t* labels, const uint8_t* present,
                   const float* grid, int* tp, int* pp, int* num, float* ent_out, int M, int B, int C, int G, void* stream);
int mla_gate_sweep_tile(int rows);
int mla_eval_head_gated(const float* x0, const float* x1, const float* x2, const float* W, const float* b, const int64_t* labels,
                        const uint8_t* present, int* counts, float* logits_out, float* fused_out, float* weights_out, int* pred_out,
                        int M, int B, int D, int C, float prior0, float prior1, float prior2, float beta, void* stream);
/* invstd = 1/sqrt(var + eps) (eval-mode BatchNorm on running statistics) */
int mla_bn_invstd(const float* var, float* invstd, int n, float eps, void* stream);

/* ---- torch.optim.SGD(momentum, weight_decay) (main.py:749, 439, 451) ------------------------- */
/* d = g + wd*p; buf = first ? d : momentum*buf + d; p -= lr*buf.  g == NULL means zero gradient
 * (torch-1.8.1 zero_grad semantics).  One flat launch over n contiguous elements; p, g and buf may
 * start at any 4-byte-aligned address (a slice flat[o:o+n] of a flat buffer): 16-byte accesses from p's first
 * 16-byte boundary on, scalar before it and after the last whole float4; all scalar when buf does not share p's
 * misalignment, dword gradient loads when only g is off.  An element's result does not depend on where the
 * range starts.  n == 0 is a no-op; a null p / buf or a pointer off a 4-byte boundary: MLA_ERR_INVALID_ARG. */
int mla_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float wd,
                 int first, void* stream);

/* ---- torch.optim.Adam (main.py:736-747 --cav_opti; main.py:31 --optimizer Adam) ---------------- */
/* amsgrad=False, maximize=False, single-tensor rule:  g' = g + wd*p;  m = beta1*m + (1-beta1)*g';
 * v = beta2*v + (1-beta2)*g'*g';  p -= (lr / (1-beta1^step)) * m / (sqrt(v)/sqrt(1-beta2^step) + eps).
 * g == NULL means zero gradient (torch-1.8.1 zero_grad semantics).  step >= 1; the caller zeroes m and v before
 * step 1.  One launch over n contiguous elements; p, g, m, v may start at any 4-byte-aligned address.  The bias corrections
 * and the step size are formed in double on the host.  Hyper-parameters travel as fp32: beta2 = 0.999 acts as
 * (double)0.999f, which moves 1-beta2 by 1.3e-5 relative in v and in its bias correction alike.
 * n == 0, a null p / m / v or step < 1: MLA_ERR_INVALID_ARG. */
int mla_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                  float wd, int step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MLA_HIP_H */
