// Latency-bound small kernels on the critical path between the two modalities:
//   shared head + cross entropy   ConcatFusion.fc_out = nn.Linear(D,C) (models/fusion_modules.py:19) applied per
//                                 modality (main.py:432, 444) + nn.CrossEntropyLoss (main.py:130) + autograd
//   head-gradient projection      GSPlugin.before_update (utils/utils.py:24-41), literal
//   SGD momentum + weight decay   torch.optim.SGD.step (main.py:749, 439, 451), one flat launch per group
// Wave-per-row kernels with 64-lane shuffle reductions; no atomics (bitwise reproducible).
#include "adam_args.h"
#include "head_common.h"

// ---- head: one workgroup per sample ------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                        float* __restrict__ logits, float* __restrict__ rowloss,
                                                        float* __restrict__ dlogits, float* __restrict__ dX, int B, int D,
                                                        int C, float inv_batch) {
  // One workgroup (4 waves) per sample.  Wave w forms the logits of classes c = w, w+4, ... (each class by ONE wave, lanes
  // striding the features: the summation order of the one-wave-per-sample form, bit-identical results), wave 0 does the
  // softmax / loss, then wave w forms dX for the feature slots d = 64 (w + 4 m) + lane.  The one-wave form was a chain of
  // C dependent reductions and C dependent row reads of W: 206 us at C = 101, D = 768 on the step's critical path.
  __shared__ float lg[MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  const float* x = X + (size_t)row * D;
  for (int c = wave; c < C; c += 4) {
    const float s = head_row_dot(x, W + (size_t)c * D, D, lane);
    if (lane == 0) lg[c] = s + bias[c];
  }
  __syncthreads();
  if (wave == 0) {
    const Softmax2 p = head_softmax2(lg, C, lane);
    const long lab_raw = (long)labels[row];
    // out of range: NaN loss (the reference's CE kernel asserts), a zero dlogits row (ce_fwd_bwd_kernel's policy), no OOB LDS read
    const bool lab_ok = lab_raw >= 0 && lab_raw < C;
    const int lab = lab_ok ? (int)lab_raw : 0;
    if (lane < C) logits[(size_t)row * C + lane] = p.l0;
    if (lane + 64 < C) logits[(size_t)row * C + lane + 64] = p.l1;
    if (lane == 0) rowloss[row] = lab_ok ? head_ce_loss(p.logs, p.mx, lg[lab]) * inv_batch : NAN;
    __builtin_amdgcn_wave_barrier();
    const float d0 = lab_ok ? head_ce_grad(p.e0, p.s, lane == lab, inv_batch) : 0.f;
    const float d1 = lab_ok ? head_ce_grad(p.e1, p.s, lane + 64 == lab, inv_batch) : 0.f;
    if (lane < C) {
      lg[lane] = d0;
      dlogits[(size_t)row * C + lane] = d0;
    }
    if (lane + 64 < C) {
      lg[lane + 64] = d1;
      dlogits[(size_t)row * C + lane + 64] = d1;
    }
  }
  __syncthreads();
  for (int d = wave * 64 + lane; d < D; d += 256) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += lg[c] * W[(size_t)c * D + d];
    dX[(size_t)row * D + d] = a;
  }
}

// Block (x, c) of a (ceil(D/256), C) grid: dW[c][d] = scale * sum_rows dl[row][c] X[row][d] (rows in order); block (0, c) also
// db[c]; `with_loss`: block (0, 0) also the loss.  The body of head_grad_kernel (the literals 1.f and true, and the loss row) and of
// head_dw_kernel (scale, false).
__device__ __forceinline__ void head_dw_block(const float* __restrict__ X, const float* __restrict__ dlogits,
                                              const float* __restrict__ rowloss, float* __restrict__ dW, float* __restrict__ db,
                                              float* __restrict__ loss, int B, int D, int C, float scale, bool with_loss) {
  const int c = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
  if (d < D) {
    float a = 0.f;
    for (int r = 0; r < B; ++r) a += dlogits[(size_t)r * C + c] * X[(size_t)r * D + d];
    dW[(size_t)c * D + d] = a * scale;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const float a = head_col_sum(dlogits, B, C, c, threadIdx.x);
    if (threadIdx.x == 0) db[c] = a * scale;
    if (with_loss && c == 0) {
      const float l = head_col_sum(rowloss, B, 1, 0, threadIdx.x);
      if (threadIdx.x == 0) *loss = l;
    }
  }
}
__global__ __launch_bounds__(256) void head_grad_kernel(const float* __restrict__ X, const float* __restrict__ dlogits,
                                                         const float* __restrict__ rowloss, float* __restrict__ dW,
                                                         float* __restrict__ db, float* __restrict__ loss, int B, int D, int C) {
  head_dw_block(X, dlogits, rowloss, dW, db, loss, B, D, C, 1.f, true);
}

extern "C" size_t mla_head_ws_elems(int B, int C) { return (size_t)B * C + B; }

extern "C" int mla_head_ce_fwd_bwd(const float* X, const float* W, const float* b, const int64_t* labels, float* logits,
                                   float* loss, float* dW, float* db, float* dX, float* ws, int B, int D, int C,
                                   float inv_batch, void* stream) {
  MLA_REQUIRE(X && W && b && labels && logits && loss && dW && db && dX && ws, "mla_head_ce_fwd_bwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0 && C <= MLA_HEAD_MAXC, "mla_head_ce_fwd_bwd: need 0 < C <= %d (got %d)", MLA_HEAD_MAXC, C);
  hipStream_t st = (hipStream_t)stream;
  float* dlogits = ws;
  float* rowloss = ws + (size_t)B * C;
  head_fwd_kernel<<<B, 256, 0, st>>>(X, W, b, labels, logits, rowloss, dlogits, dX, B, D, C, inv_batch);
  MLA_CHECK_LAUNCH("head_fwd_kernel");
  head_grad_kernel<<<dim3(cdiv(D, 256), C), 256, 0, st>>>(X, dlogits, rowloss, dW, db, loss, B, D, C);
  MLA_CHECK_LAUNCH("head_grad_kernel");
  return MLA_OK;
}

// ---- autograd-protocol entry points: the same head, split where autograd splits it (main.py:432-435) -------------
// nn.CrossEntropyLoss (mean) forward + d logits in one launch: one wave per sample.  A label outside [0, C) poisons
// the loss with NaN (the reference's CUDA kernel asserts); its d logits row is zero.
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                          float* __restrict__ rowloss, float* __restrict__ dlogits, int B, int C,
                                                          float inv_batch) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const float* l = logits + (size_t)row * C;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, l[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(l[c] - m);
  s = wave_sum(s);
  const long lab = (long)labels[row];
  const bool ok = lab >= 0 && lab < C;
  if (lane == 0) rowloss[row] = ok ? head_ce_loss(logf(s), m, l[lab]) * inv_batch : NAN;
  for (int c = lane; c < C; c += 64)
    dlogits[(size_t)row * C + c] = ok ? (expf(l[c] - m) / s - (c == lab ? 1.f : 0.f)) * inv_batch : 0.f;
}
__global__ __launch_bounds__(64) void sum_to_scalar_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
  const float a = head_col_sum(v, n, 1, 0, threadIdx.x);
  if (threadIdx.x == 0) *out = a;
}
extern "C" int mla_ce_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits, float* ws, int B, int C,
                              float inv_batch, void* stream) {
  MLA_REQUIRE(logits && labels && loss && dlogits && ws && B > 0 && C > 0, "mla_ce_fwd_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  ce_fwd_bwd_kernel<<<cdiv(B, 4), 256, 0, st>>>(logits, labels, ws, dlogits, B, C, inv_batch);
  MLA_CHECK_LAUNCH("ce_fwd_bwd_kernel");
  sum_to_scalar_kernel<<<1, 64, 0, st>>>(ws, loss, B);
  MLA_CHECK_LAUNCH("sum_to_scalar_kernel");
  return MLA_OK;
}

// nn.Linear backward from an arbitrary d logits (autograd hands it over): dX = scale * dl W (wave per sample),
// dW = scale * dl^T X, db = scale * colsum(dl).  scale = 1/world under data parallel.
__global__ __launch_bounds__(256) void head_dx_kernel(const float* __restrict__ dlogits, const float* __restrict__ W,
                                                       float* __restrict__ dX, int B, int D, int C, float scale) {
  const int d = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (d >= D) return;
  float a = 0.f;
  for (int c = 0; c < C; ++c) a += dlogits[(size_t)row * C + c] * W[(size_t)c * D + d];
  dX[(size_t)row * D + d] = a * scale;
}
__global__ __launch_bounds__(256) void head_dw_kernel(const float* __restrict__ X, const float* __restrict__ dlogits,
                                                       float* __restrict__ dW, float* __restrict__ db, int B, int D, int C,
                                                       float scale) {
  head_dw_block(X, dlogits, nullptr, dW, db, nullptr, B, D, C, scale, false);
}
extern "C" int mla_head_bwd(const float* X, const float* W, const float* dlogits, float* dW, float* db, float* dX, int B, int D,
                            int C, float scale, void* stream) {
  MLA_REQUIRE(X && W && dlogits && dW && db && dX && B > 0 && D > 0 && C > 0, "mla_head_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  head_dx_kernel<<<dim3(cdiv(D, 256), B), 256, 0, st>>>(dlogits, W, dX, B, D, C, scale);
  MLA_CHECK_LAUNCH("head_dx_kernel");
  head_dw_kernel<<<dim3(cdiv(D, 256), C), 256, 0, st>>>(X, dlogits, dW, db, B, D, C, scale);
  MLA_CHECK_LAUNCH("head_dw_kernel");
  return MLA_OK;
}

// x[i] *= *scalar (the scalar lives on the device: the gradient autograd passes into a loss node)
__global__ __launch_bounds__(256) void scale_dev_kernel(float* __restrict__ x, const float* __restrict__ s, size_t n) {
  const float f = *s;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) x[i] *= f;
}
extern "C" int mla_scale_by_device_scalar(float* x, const float* scalar, size_t n, void* stream) {
  MLA_REQUIRE(x && scalar, "mla_scale_by_device_scalar: null pointer");
  if (n == 0) return MLA_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  scale_dev_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(x, scalar, n);
  MLA_CHECK_LAUNCH("scale_dev_kernel");
  return MLA_OK;
}

// ---- column sum ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, float* __restrict__ r, int B, int D, float scale) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float a = 0.f;
  for (int i = 0; i < B; ++i) a += X[(size_t)i * D + d];
  r[d] = a * scale;
}

extern "C" int mla_colsum(const float* X, float* r, int B, int D, float scale, void* stream) {
  MLA_REQUIRE(X && r && B > 0 && D > 0, "mla_colsum: bad argument");
  colsum_kernel<<<cdiv(D, 256), 256, 0, (hipStream_t)stream>>>(X, r, B, D, scale);
  MLA_CHECK_LAUNCH("colsum_kernel");
  return MLA_OK;
}

// ---- GS projection: three row-parallel phases (wave per row of Pl) ---------------------------------
// A: k = Pl r^T
__global__ __launch_bounds__(256) void gs_k_kernel(const float* __restrict__ Pl, const float* __restrict__ r,
                                                    float* __restrict__ k, int D) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= D) return;
  float s = 0.f;
  for (int j = lane; j < D; j += 64) s += Pl[(size_t)i * D + j] * r[j];
  s = wave_sum(s);
  if (lane == 0) k[i] = s;
}
// B: Pl[i][j] -= k_i k_j / (alpha + k_i r_j)   (element-wise DxD denominator, utils/utils.py:36); row sums of squares
__global__ __launch_bounds__(256) void gs_update_kernel(float* __restrict__ Pl, const float* __restrict__ r,
                                                         const float* __restrict__ k, float* __restrict__ rowsq, int D,
                                                         float alpha) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= D) return;
  const float ki = k[i];
  float q = 0.f;
  for (int j = lane; j < D; j += 64) {
    const float v = Pl[(size_t)i * D + j] - (ki * k[j]) / (alpha + ki * r[j]);
    Pl[(size_t)i * D + j] = v;
    q += v * v;
  }
  q = wave_sum(q);
  if (lane == 0) rowsq[i] = q;
}
// C: Pl /= ||Pl||_F ; Gout[c][i] = sum_j G[c][j] Pl[i][j]
// One workgroup (4 waves) per row of Pl: every wave forms the norm (same order: bit-identical), wave w normalises the columns
// j = 64 (w + 4 m) + lane and, after a barrier, projects the classes c = w, w+4, ... (each class by one wave in the lane / stride
// order of the one-wave-per-row form).  At C = 101 that form was a chain of 101 dependent reductions per row: 300 us.
__global__ __launch_bounds__(256) void gs_finish_kernel(float* __restrict__ Pl, const float* __restrict__ rowsq,
                                                         const float* __restrict__ G, float* __restrict__ Gout, int D, int C) {
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double t = 0.0;
  for (int j = lane; j < D; j += 64) t += (double)rowsq[j];
  t = wave_sum_d(t);
  const float nrm = (float)sqrt(t);
  for (int j = wave * 64 + lane; j < D; j += 256) Pl[(size_t)i * D + j] = Pl[(size_t)i * D + j] / nrm;
  __syncthreads();                       // the row is complete (and visible to the workgroup) before it is read back
  for (int c = wave; c < C; c += 4) {
    float s = 0.f;
    for (int j = lane; j < D; j += 64) s += G[(size_t)c * D + j] * Pl[(size_t)i * D + j];
    s = wave_sum(s);
    if (lane == 0) Gout[(size_t)c * D + i] = s;
  }
}

extern "C" size_t mla_gs_ws_elems(int D, int C) { return (size_t)2 * D + (size_t)C * D; }

extern "C" int mla_gs_project(float* Pl, const float* r, float* G, int D, int C, float alpha, float* ws, void* stream) {
  MLA_REQUIRE(Pl && r && G && ws && D > 0 && C > 0, "mla_gs_project: bad argument");
  hipStream_t st = (hipStream_t)stream;
  float *k = ws, *rowsq = ws + D, *Gtmp = ws + 2 * (size_t)D;
  gs_k_kernel<<<cdiv(D, 4), 256, 0, st>>>(Pl, r, k, D);
  MLA_CHECK_LAUNCH("gs_k_kernel");
  gs_update_kernel<<<cdiv(D, 4), 256, 0, st>>>(Pl, r, k, rowsq, D, alpha);
  MLA_CHECK_LAUNCH("gs_update_kernel");
  gs_finish_kernel<<<D, 256, 0, st>>>(Pl, rowsq, G, Gtmp, D, C);
  MLA_CHECK_LAUNCH("gs_finish_kernel");
  if (hipMemcpyAsync(G, Gtmp, (size_t)C * D * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    mla_set_error("mla_gs_project: hipMemcpyAsync failed");
    return MLA_ERR_LAUNCH;
  }
  return MLA_OK;
}

// ---- SGD -------------------------------------------------------------------------------------------
// The float4 body starts at p's first 16-byte boundary (`head` elements in) and covers n4 groups; the elements before it and after
// its last whole float4 are scalar (adam_args.h: range_plan; p and buf of a slice flat[o:o+n] share their misalignment).  GVEC:
// the gradient is aligned with p too; otherwise it takes four dword loads per float4.  On the all-scalar launch n4 is 0.
template <bool GVEC>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                   size_t n, size_t head, size_t n4, float lr, float momentum, float wd, int first) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + head);
  f32x4* b4 = reinterpret_cast<f32x4*>(buf + head);
  for (size_t i = tid; i < n4; i += nthr) {
    f32x4 pv = p4[i];
    f32x4 d = pv * wd;
    if (g) {
      if constexpr (GVEC) {
        d += reinterpret_cast<const f32x4*>(g + head)[i];
      } else {
        const float* gs = g + head + 4 * i;
        d += f32x4{gs[0], gs[1], gs[2], gs[3]};
      }
    }
    f32x4 b = first ? d : b4[i] * momentum + d;
    b4[i] = b;
    p4[i] = pv - b * lr;
  }
  // everything outside the float4 body: [0, head) and [head + 4 n4, n) (at most 6 elements; all of n on the scalar launch)
  const size_t rest = n - 4 * n4;
  for (size_t r = tid; r < rest; r += nthr) {         // sgd_elem's expression (head_common.h), with g == nullptr as a zero gradient
    const size_t i = r < head ? r : r + 4 * n4;
    const float pv = p[i];
    const float d = (g ? g[i] : 0.f) + wd * pv;
    const float b = first ? d : momentum * buf[i] + d;
    buf[i] = b;
    p[i] = pv - lr * b;
  }
}

extern "C" int mla_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float wd, int first,
                            void* stream) {
  MLA_REQUIRE(p && buf, "mla_sgd_step: null pointer");
  if (n == 0) return MLA_OK;
  RangePlan pl;
  MLA_REQUIRE(range_plan(p, g, buf, nullptr, n, &pl), "mla_sgd_step: buffers must be 4-byte aligned");
  size_t blocks = ((pl.vec ? pl.n4 : n) + 255) / 256;         // threads' worth of grid-stride work
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  if (pl.gvec)
    sgd_kernel<true><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(p, g, buf, n, pl.head, pl.n4, lr, momentum, wd, first);
  else
    sgd_kernel<false><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(p, g, buf, n, pl.head, pl.n4, lr, momentum, wd, first);
  MLA_CHECK_LAUNCH("sgd_kernel");
  return MLA_OK;
}

// invstd[i] = 1 / sqrt(var[i] + eps): eval-mode BatchNorm uses the running statistics (one launch per encoder over
// its flat running_var buffer)
__global__ __launch_bounds__(256) void invstd_kernel(const float* __restrict__ var, float* __restrict__ invstd, int n, float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) invstd[i] = 1.0f / sqrtf(var[i] + eps);
}
extern "C" int mla_bn_invstd(const float* var, float* invstd, int n, float eps, void* stream) {
  MLA_REQUIRE(var && invstd && n > 0, "mla_bn_invstd: bad argument");
  invstd_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(var, invstd, n, eps);
  MLA_CHECK_LAUNCH("invstd_kernel");
  return MLA_OK;
}
