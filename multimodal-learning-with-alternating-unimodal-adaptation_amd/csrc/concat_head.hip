// Concatenated fusion head of the joint (non --gs_flag) step: ConcatFusion.fc_out = nn.Linear(M*D, C) applied to
// cat(x_1 .. x_M) (models/fusion_modules.py:16-35), the half / third-head logits of main.py:283-302, the training loss
// nn.CrossEntropyLoss (main.py:305) with its gradients, and the reported (never differentiated) per-modality losses
// (main.py:307-309).  The M feature buffers are read in place: the concatenation is never materialised; column block m of
// W (C x M*D, row-major, the reference's layout) multiplies modality m.
//
// Latency-bound at the step's shapes (64 x 1024 x 6): few launches, wave-per-class dot products with 64-lane shuffle
// reductions, no atomics, every sum in a fixed order (bitwise reproducible from run to run).
#include "head_common.h"

namespace {

struct ConcatPtrs {
  const float* x[MLA_HEAD_MAXM];   // (B, D) features of modality m
  float* dx[MLA_HEAD_MAXM];        // (B, D) feature gradients (backward variants)
};

// One workgroup (4 waves) per sample.  Wave w forms the logits of classes c = w, w + 4, ...: for every modality the partial
// product s_m = x_m . W[c, mD : (m+1)D] (lanes stride the features), out = s_0 + s_1 (+ s_2) + b, out_m = s_m + b / M.
// TRAIN: wave 0 then forms softmax / CE / dlogits of `out`, waves 1..M the CE of out_m (reported losses), and after a
// barrier the workgroup forms dX_m[d] = sum_c dlogits[c] W[c, mD + d] for all M*D feature slots.
template <bool TRAIN>
__global__ __launch_bounds__(256) void concat_head_fwd_kernel(const ConcatPtrs p, const float* __restrict__ W,
                                                               const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                               float* __restrict__ out, float* __restrict__ out_m,
                                                               float* __restrict__ dlogits, float* __restrict__ rowloss, int M,
                                                               int B, int D, int C, float inv_batch) {
  __shared__ float lg[MLA_HEAD_MAXC];
  __shared__ float lgm[MLA_HEAD_MAXM][MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  const int MD = M * D;
  const float invM = 1.f / (float)M;
  for (int c = wave; c < C; c += 4) {
    const float* w = W + (size_t)c * MD;
    float tot = 0.f;
    for (int m = 0; m < M; ++m) {
      const float* x = p.x[m] + (size_t)row * D;
      const float s = head_row_dot(x, w + (size_t)m * D, D, lane);
      tot += s;
      const float om = s + bias[c] * invM;                               // main.py:298-302: + fc_out.bias / 2 (/ 3)
      if (lane == 0) {
        out_m[((size_t)m * B + row) * C + c] = om;
        lgm[m][c] = om;
      }
    }
    const float o = tot + bias[c];
    if (lane == 0) {
      out[(size_t)row * C + c] = o;
      lg[c] = o;
    }
  }
  if (!TRAIN) return;
  __syncthreads();
  const long lab_raw = (long)labels[row];
  const bool lab_ok = lab_raw >= 0 && lab_raw < C;    // out of range: NaN loss (the reference's CE kernel asserts), zero dlogits
  const int lab = lab_ok ? (int)lab_raw : 0;
  if (wave <= M) {
    // wave 0: the trained logits `out`; wave 1 + m: out_m (loss value only)
    const float* l = wave == 0 ? lg : lgm[wave - 1];
    const Softmax2 q = head_softmax2(l, C, lane);
    if (lane == 0) rowloss[(size_t)wave * B + row] = lab_ok ? head_ce_loss(q.logs, q.mx, l[lab]) * inv_batch : NAN;
    if (wave == 0) {
      __builtin_amdgcn_wave_barrier();              // every lane has read lg before it is overwritten with dlogits
      const float d0 = lab_ok ? head_ce_grad(q.e0, q.s, lane == lab, inv_batch) : 0.f;
      const float d1 = lab_ok ? head_ce_grad(q.e1, q.s, lane + 64 == lab, inv_batch) : 0.f;
      if (lane < C) {
        lg[lane] = d0;
        dlogits[(size_t)row * C + lane] = d0;
      }
      if (lane + 64 < C) {
        lg[lane + 64] = d1;
        dlogits[(size_t)row * C + lane + 64] = d1;
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < MD; j += 256) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += lg[c] * W[(size_t)c * MD + j];
    const int m = j / D;
    p.dx[m][(size_t)row * D + (j - m * D)] = a;
  }
}

// dX_m = scale * dlogits W_m for a given dlogits (the autograd backward): grid (ceil(M*D / 256), B)
__global__ __launch_bounds__(256) void concat_head_dx_kernel(const ConcatPtrs p, const float* __restrict__ W,
                                                              const float* __restrict__ dlogits, int M, int B, int D, int C,
                                                              float scale) {
  const int MD = M * D;
  const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (j >= MD) return;
  float a = 0.f;
  for (int c = 0; c < C; ++c) a += dlogits[(size_t)row * C + c] * W[(size_t)c * MD + j];
  const int m = j / D;
  p.dx[m][(size_t)row * D + (j - m * D)] = a * scale;
}

// grid (ceil(M*D / 256), C): dW[c][j] = scale * sum_rows dlogits[row][c] x_{j/D}[row][j%D] (rows in order); block (0, c) also
// db[c]; with `rowloss`, block (0, 0) sums the M + 1 loss rows (training loss, then the per-modality losses).
__global__ __launch_bounds__(256) void concat_head_dw_kernel(const ConcatPtrs p, const float* __restrict__ dlogits,
                                                              const float* __restrict__ rowloss, float* __restrict__ dW,
                                                              float* __restrict__ db, float* __restrict__ loss,
                                                              float* __restrict__ loss_m, int M, int B, int D, int C,
                                                              float scale) {
  const int MD = M * D;
  const int c = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j < MD) {
    const int m = j / D;
    const float* x = p.x[m] + (j - m * D);
    float a = 0.f;
    for (int r = 0; r < B; ++r) a += dlogits[(size_t)r * C + c] * x[(size_t)r * D];
    dW[(size_t)c * MD + j] = a * scale;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const float a = head_col_sum(dlogits, B, C, c, threadIdx.x);
    if (threadIdx.x == 0) db[c] = a * scale;
    if (c == 0 && rowloss) {
      for (int k = 0; k <= M; ++k) {
        const float l = head_col_sum(rowloss + (size_t)k * B, B, 1, 0, threadIdx.x);
        if (threadIdx.x == 0) {
          if (k == 0) *loss = l;
          else loss_m[k - 1] = l;
        }
      }
    }
  }
}

ConcatPtrs make_ptrs(const float* x0, const float* x1, const float* x2, float* dx0, float* dx1, float* dx2) {
  ConcatPtrs p;
  p.x[0] = x0; p.x[1] = x1; p.x[2] = x2;
  p.dx[0] = dx0; p.dx[1] = dx1; p.dx[2] = dx2;
  return p;
}

}  // namespace

extern "C" size_t mla_concat_head_ws_elems(int B, int C, int M) { return (size_t)B * C + (size_t)B * (M + 1); }

extern "C" int mla_concat_head_ce_fwd_bwd(const float* x0, const float* x1, const float* x2, const float* W, const float* b,
                                          const int64_t* labels, float* out, float* out_m, float* loss, float* loss_m, float* dW,
                                          float* db, float* dx0, float* dx1, float* dx2, float* ws, int M, int B, int D, int C,
                                          float inv_batch, void* stream) {
  MLA_REQUIRE(M == 2 || M == 3, "mla_concat_head_ce_fwd_bwd: M must be 2 or 3 (got %d)", M);
  MLA_REQUIRE(x0 && x1 && (M == 2 || x2) && W && b && labels && out && out_m && loss && loss_m && dW && db && dx0 && dx1 &&
                  (M == 2 || dx2) && ws,
              "mla_concat_head_ce_fwd_bwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0 && C <= MLA_HEAD_MAXC, "mla_concat_head_ce_fwd_bwd: need B, D > 0 and 0 < C <= %d (got %d)",
              MLA_HEAD_MAXC, C);
  hipStream_t st = (hipStream_t)stream;
  const ConcatPtrs p = make_ptrs(x0, x1, M == 3 ? x2 : nullptr, dx0, dx1, M == 3 ? dx2 : nullptr);
  float* dlogits = ws;
  float* rowloss = ws + (size_t)B * C;
  concat_head_fwd_kernel<true><<<B, 256, 0, st>>>(p, W, b, labels, out, out_m, dlogits, rowloss, M, B, D, C, inv_batch);
  MLA_CHECK_LAUNCH("concat_head_fwd_kernel<train>");
  concat_head_dw_kernel<<<dim3(cdiv((long)M * D, 256), C), 256, 0, st>>>(p, dlogits, rowloss, dW, db, loss, loss_m, M, B, D, C,
                                                                         1.f);
  MLA_CHECK_LAUNCH("concat_head_dw_kernel");
  return MLA_OK;
}

extern "C" int mla_concat_head_fwd(const float* x0, const float* x1, const float* x2, const float* W, const float* b, float* out,
                                   float* out_m, int M, int B, int D, int C, void* stream) {
  MLA_REQUIRE(M == 2 || M == 3, "mla_concat_head_fwd: M must be 2 or 3 (got %d)", M);
  MLA_REQUIRE(x0 && x1 && (M == 2 || x2) && W && b && out && out_m, "mla_concat_head_fwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0 && C <= MLA_HEAD_MAXC, "mla_concat_head_fwd: need B, D > 0 and 0 < C <= %d (got %d)", MLA_HEAD_MAXC, C);
  const ConcatPtrs p = make_ptrs(x0, x1, M == 3 ? x2 : nullptr, nullptr, nullptr, nullptr);
  concat_head_fwd_kernel<false><<<B, 256, 0, (hipStream_t)stream>>>(p, W, b, nullptr, out, out_m, nullptr, nullptr, M, B, D, C,
                                                                    0.f);
  MLA_CHECK_LAUNCH("concat_head_fwd_kernel");
  return MLA_OK;
}

extern "C" int mla_concat_head_bwd(const float* x0, const float* x1, const float* x2, const float* W, const float* dlogits,
                                   float* dW, float* db, float* dx0, float* dx1, float* dx2, int M, int B, int D, int C,
                                   float scale, void* stream) {
  MLA_REQUIRE(M == 2 || M == 3, "mla_concat_head_bwd: M must be 2 or 3 (got %d)", M);
  MLA_REQUIRE(x0 && x1 && (M == 2 || x2) && W && dlogits && dW && db && dx0 && dx1 && (M == 2 || dx2),
              "mla_concat_head_bwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0, "mla_concat_head_bwd: bad shape");
  hipStream_t st = (hipStream_t)stream;
  const ConcatPtrs p = make_ptrs(x0, x1, M == 3 ? x2 : nullptr, dx0, dx1, M == 3 ? dx2 : nullptr);
  concat_head_dx_kernel<<<dim3(cdiv((long)M * D, 256), B), 256, 0, st>>>(p, W, dlogits, M, B, D, C, scale);
  MLA_CHECK_LAUNCH("concat_head_dx_kernel");
  concat_head_dw_kernel<<<dim3(cdiv((long)M * D, 256), C), 256, 0, st>>>(p, dlogits, nullptr, dW, db, nullptr, nullptr, M, B, D, C,
                                                                         scale);
  MLA_CHECK_LAUNCH("concat_head_dw_kernel");
  return MLA_OK;
}
