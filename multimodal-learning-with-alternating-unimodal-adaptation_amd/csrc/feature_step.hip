// The head-only modality phase of a model that trains on stored features (CLIPClassifier, models/basic_model.py:278-319): there
// is no encoder behind the features, so one phase of main.py:432-442 is fc_out -> cross entropy -> GSPlugin.before_update
// (utils/utils.py:24-41) -> SGD on the head and nothing else.  On the general chain (head_gs_sgd.hip) that is 7 launches and a
// device-to-device copy, and a dX nobody reads.  Here it is 4 launches (2 when the projection does not fire), no copy, no dX,
// and the projected gradient never reaches memory: the launch that forms column i of G Pl^T applies SGD to W[:, i] from registers.
//
//   1. feat_fwd_kernel     logits, softmax, row loss, dlogits                      one workgroup per sample
//   2. feat_grad_kernel    dW, db (+ bias SGD), loss; projecting: r = mean(X, 0), k = Pl r^T, dW -> workspace
//                          not projecting: SGD on W from registers (this launch never reads W)
//   3. feat_rowsq_kernel   row sums of squares of Pl[i][j] - k_i k_j / (alpha + k_i r_j)                     (projecting only)
//   4. feat_finish_kernel  that row again, / ||.||_F, stored; g_c = sum_j G[c][j] Pl[i][j]; SGD on W[c][i]   (projecting only)
//
// Grid dependencies are kernel boundaries: no cooperative launch, no flag another workgroup waits on, no atomics.  Head and cross
// entropy are written on the chain's helpers (head_common.h: head_row_dot, head_softmax2, head_ce_grad, head_col_sum; dW sums its rows
// in order, as head_dw_block does): logits and loss are the chain's bit for bit.  The projection is the literal utils/utils.py:34-41
// in the chain's lane / stride order, but r, k, the denominator, the norm and the projected sums are carried in fp64 and every stored value is rounded once: with features
// of both signs some denominators come within a few hundred ulp of zero, where an fp32 r or k decides the answer.
// mla_feature_phase_owm is the same phase with the scalar-denominator rule of gs_owm.hip in fp32: launches 1 and 2 (r and k in fp32),
// no rowsq launch, and feat_finish_owm_kernel in place of 4 -- 3 launches when it projects.
// Also here: mla_gather_rows2, the batch feed of such a model from device-resident feature tables (dataset/dataset.py:864-872).
#include "head_common.h"
#include "feature_args.h"

// Waves per workgroup of the two launches that walk the classes (1 and 4).  Each class is still formed by ONE wave with lanes striding
// the features (head_row_dot); 16 waves instead of the chain's 4 shorten the chain of dependent row reads and
// reductions per wave from ceil(C / 4) to ceil(C / 16).
#define FEAT_WAVES 16

// ---- 1. head forward + softmax + d logits on the helpers of head_common.h (head_fwd_kernel without its dX half) -----------
__global__ __launch_bounds__(64 * FEAT_WAVES) void feat_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                        const float* __restrict__ bias, const int64_t* __restrict__ labels,
                                                        float* __restrict__ logits, float* __restrict__ rowloss,
                                                        float* __restrict__ dlogits, int D, int C, float inv_batch) {
  __shared__ float lg[MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  const float* x = X + (size_t)row * D;
  for (int c = wave; c < C; c += FEAT_WAVES) {
    const float s = head_row_dot(x, W + (size_t)c * D, D, lane);
    if (lane == 0) lg[c] = s + bias[c];
  }
  __syncthreads();
  if (wave != 0) return;
  const Softmax2 p = head_softmax2(lg, C, lane);
  const long lab_raw = (long)labels[row];
  const bool lab_ok = lab_raw >= 0 && lab_raw < C;   // out of range: NaN loss, a zero dlogits row, no out-of-bounds LDS read
  const int lab = lab_ok ? (int)lab_raw : 0;
  if (lane == 0) rowloss[row] = lab_ok ? head_ce_loss(p.logs, p.mx, lg[lab]) * inv_batch : NAN;
  const float d0 = lab_ok ? head_ce_grad(p.e0, p.s, lane == lab, inv_batch) : 0.f;
  const float d1 = lab_ok ? head_ce_grad(p.e1, p.s, lane + 64 == lab, inv_batch) : 0.f;
  if (lane < C) {
    logits[(size_t)row * C + lane] = p.l0;
    dlogits[(size_t)row * C + lane] = d0;
  }
  if (lane + 64 < C) {
    logits[(size_t)row * C + lane + 64] = p.l1;
    dlogits[(size_t)row * C + lane + 64] = d1;
  }
}

struct FeatGradArgs {
  const float* X;
  const float* dlogits;
  const float* rowloss;
  const float* Pl;
  float *W, *b, *bufW, *bufb;     // updated in place
  float *G, *loss;                // out
  double *r, *k;                  // out (projecting)
  float *r32, *k32;               // out (projecting, the scalar-denominator rule: fp32)
  int B, D, C, dchunks, grad_blocks, project, first;
  float inv_batch, lr, momentum, wd;
};

// ---- 2. blocks [0, grad_blocks): dW[c][d] = sum_rows dl[row][c] X[row][d] (rows in order, as head_dw_block); the d-chunk-0 block
// of class c also db[c] and the bias SGD, the one of class 0 the loss.  Blocks past them (projecting): r = mean(X, 0) into LDS in
// fp64 (every block its own copy, rows in order; block 0 of them publishes it), then k_i = Pl[i] . r for FEATURE_KROWS rows of Pl
// (one wave per row, lanes striding the columns, fp64 accumulators).  OWM (mla_feature_phase_owm): the same blocks in fp32, r as
// colsum_kernel forms it (rows in order, times 1 / B) and k as gs_owm_k_kernel does; everything else is the same text.
template <bool OWM>
__global__ __launch_bounds__(256) void feat_grad_kernel(const FeatGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) double r_s[];
  const int B = a.B, D = a.D, C = a.C;
  if ((int)blockIdx.x >= a.grad_blocks) {
    const int kb = blockIdx.x - a.grad_blocks;
    if constexpr (OWM) {
      float* r32_s = reinterpret_cast<float*>(r_s);
      const float inv_b = 1.f / (float)B;
      for (int d = threadIdx.x; d < D; d += 256) {
        float s = 0.f;
        for (int i = 0; i < B; ++i) s += a.X[(size_t)i * D + d];
        s = s * inv_b;
        r32_s[d] = s;
        if (kb == 0) a.r32[d] = s;
      }
      __syncthreads();
      const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
      for (int q = wave; q < FEATURE_KROWS; q += 4) {
        const int i = kb * FEATURE_KROWS + q;
        if (i >= D) break;
        float s = 0.f;
        for (int j = lane; j < D; j += 64) s += a.Pl[(size_t)i * D + j] * r32_s[j];
        s = wave_sum(s);
        if (lane == 0) a.k32[i] = s;
      }
      return;
    }
    for (int d = threadIdx.x; d < D; d += 256) {
      double s = 0.0;
      for (int i = 0; i < B; ++i) s += (double)a.X[(size_t)i * D + d];
      s = s / (double)B;
      r_s[d] = s;
      if (kb == 0) a.r[d] = s;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = wave; q < FEATURE_KROWS; q += 4) {
      const int i = kb * FEATURE_KROWS + q;
      if (i >= D) break;
      double s = 0.0;
      for (int j = lane; j < D; j += 64) s += (double)a.Pl[(size_t)i * D + j] * r_s[j];
      s = wave_sum_d(s);
      if (lane == 0) a.k[i] = s;
    }
    return;
  }
  const int c = blockIdx.x / a.dchunks, chunk = blockIdx.x - c * a.dchunks;
  const int d = chunk * 256 + threadIdx.x;
  if (d < D) {
    float g = 0.f;
    for (int r = 0; r < B; ++r) g += a.dlogits[(size_t)r * C + c] * a.X[(size_t)r * D + d];
    const size_t e = (size_t)c * D + d;
    if (a.project) a.G[e] = g;
    else sgd_elem(a.W + e, a.bufW + e, g, a.lr, a.momentum, a.wd, a.first);
  }
  if (chunk == 0 && threadIdx.x < 64) {
    const float g = head_col_sum(a.dlogits, B, C, c, threadIdx.x);
    if (threadIdx.x == 0) sgd_elem(a.b + c, a.bufb + c, g, a.lr, a.momentum, a.wd, a.first);
    if (c == 0) {
      const float l = head_col_sum(a.rowloss, B, 1, 0, threadIdx.x);
      if (threadIdx.x == 0) *a.loss = l;
    }
  }
}

// The updated, not yet normalised element (utils/utils.py:36, element-wise D x D denominator), in fp64 from the fp32 Pl.
__device__ __forceinline__ double pl_update(float pl, double ki, double kj, double rj, double alpha) {
  return (double)pl - (ki * kj) / (alpha + ki * rj);
}

// ---- 3. row sums of squares of the updated Pl (one wave per row); Pl itself is not written here: launch 4 forms its row again and
// rounds it once, after the normalisation.
__global__ __launch_bounds__(256) void feat_rowsq_kernel(const float* __restrict__ Pl, const double* __restrict__ r,
                                                          const double* __restrict__ k, double* __restrict__ rowsq, int D, double alpha) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= D) return;
  const double ki = k[i];
  double q = 0.0;
  for (int j = lane; j < D; j += 64) {
    const double v = pl_update(Pl[(size_t)i * D + j], ki, k[j], r[j], alpha);
    q += v * v;
  }
  q = wave_sum_d(q);
  if (lane == 0) rowsq[i] = q;
}

// ---- 4. one workgroup per row i of Pl: the Frobenius norm, the updated and normalised row to memory and to LDS (fp32, rounded once),
// then wave w forms column i of G Pl^T for the classes c = w, w + FEAT_WAVES, ... (lanes striding the columns, fp64 accumulator) and its
// lane 0 applies SGD to W[c][i]: the projected gradient lives in that one register.  Row i of the old Pl is read by this workgroup only.
__global__ __launch_bounds__(64 * FEAT_WAVES) void feat_finish_kernel(float* __restrict__ Pl, const double* __restrict__ r,
                                                           const double* __restrict__ k, const double* __restrict__ rowsq,
                                                           const float* __restrict__ G, float* __restrict__ W, float* __restrict__ bufW,
                                                           int D, int C, double alpha, float lr, float momentum, float wd, int first) {
  extern __shared__ __attribute__((aligned(16))) float row_s[];
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double t = 0.0;
  for (int j = lane; j < D; j += 64) t += rowsq[j];
  t = wave_sum_d(t);
  const double nrm = sqrt(t);
  const double ki = k[i];
  for (int j = threadIdx.x; j < D; j += 64 * FEAT_WAVES) {
    const float v = (float)(pl_update(Pl[(size_t)i * D + j], ki, k[j], r[j], alpha) / nrm);
    Pl[(size_t)i * D + j] = v;
    row_s[j] = v;
  }
  __syncthreads();
  for (int c = wave; c < C; c += FEAT_WAVES) {
    double s = 0.0;
    for (int j = lane; j < D; j += 64) s += (double)G[(size_t)c * D + j] * (double)row_s[j];
    s = wave_sum_d(s);
    if (lane == 0) {
      const size_t e = (size_t)c * D + i;
      sgd_elem(W + e, bufW + e, (float)s, lr, momentum, wd, first);
    }
  }
}

// ---- 3 + 4 of the scalar-denominator rule (mla_feature_phase_owm; gs_owm.hip states the rule): one workgroup per row i of Pl.  Every
// wave forms s = alpha + r . k in the same lane / stride order (the same bits in every wave and workgroup); the workgroup updates row i
// as Pl[i][j] - (k_i * k_j) / s (symmetric in (i, j)), stores it and keeps it in LDS; wave w then forms column i of G Pl^T for the
// classes c = w, w + FEAT_WAVES, ... and its lane 0 applies SGD to W[c][i].  fp32 throughout: s >= alpha is well away from zero.
__global__ __launch_bounds__(64 * FEAT_WAVES) void feat_finish_owm_kernel(float* __restrict__ Pl, const float* __restrict__ r,
                                                               const float* __restrict__ k, const float* __restrict__ G,
                                                               float* __restrict__ W, float* __restrict__ bufW, int D, int C,
                                                               float alpha, float lr, float momentum, float wd, int first) {
  extern __shared__ __attribute__((aligned(16))) float row_s[];
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float t = 0.f;
  for (int j = lane; j < D; j += 64) t += r[j] * k[j];
  const float s = alpha + wave_sum(t);
  const float ki = k[i];
  for (int j = threadIdx.x; j < D; j += 64 * FEAT_WAVES) {
    const float v = Pl[(size_t)i * D + j] - (ki * k[j]) / s;
    Pl[(size_t)i * D + j] = v;
    row_s[j] = v;
  }
  __syncthreads();
  for (int c = wave; c < C; c += FEAT_WAVES) {
    float g = 0.f;
    for (int j = lane; j < D; j += 64) g += G[(size_t)c * D + j] * row_s[j];
    g = wave_sum(g);
    if (lane == 0) {
      const size_t e = (size_t)c * D + i;
      sgd_elem(W + e, bufW + e, g, lr, momentum, wd, first);
    }
  }
}

extern "C" size_t mla_feature_ws_elems(int B, int D, int C) { return feature_ws_elems(B, D, C); }

// Both entry points: launches 1 and 2, then -- when the projection fires -- the literal rule's rowsq and finish launches in fp64
// (OWM false: r | k | rowsq, D doubles each, in the workspace's fp64 region) or the scalar rule's one finish launch in fp32 (OWM
// true: r | k, D floats each, at the head of that region).
template <bool OWM>
static int feature_phase_run(const char* who, const float* X, const int64_t* labels, float* W, float* b, float* buf, float* Pl,
                             float* logits, float* loss, float* ws, int B, int D, int C, float inv_batch, int project, double alpha,
                             float lr, float momentum, float wd, int first, void* stream) {
  FeaturePlan p;
  const int rc = feature_phase_plan_for(who, X, labels, W, b, buf, Pl, logits, loss, ws, B, D, C, project, &p);
  if (rc != MLA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  feat_fwd_kernel<<<B, 64 * FEAT_WAVES, 0, st>>>(X, W, b, labels, logits, ws + p.rowloss, ws + p.dlogits, D, C, inv_batch);
  MLA_CHECK_LAUNCH("feat_fwd_kernel");
  FeatGradArgs a;
  a.X = X; a.dlogits = ws + p.dlogits; a.rowloss = ws + p.rowloss; a.Pl = Pl;
  a.W = W; a.b = b; a.bufW = buf; a.bufb = buf + (size_t)C * D;
  double* w64 = reinterpret_cast<double*>(ws + p.f64);
  float* w32 = ws + p.f64;
  a.G = ws + p.G; a.loss = loss;
  a.r = OWM ? nullptr : w64; a.k = OWM ? nullptr : w64 + D;
  a.r32 = OWM ? w32 : nullptr; a.k32 = OWM ? w32 + D : nullptr;
  a.B = B; a.D = D; a.C = C; a.dchunks = p.dchunks; a.grad_blocks = p.grad_blocks; a.project = project ? 1 : 0; a.first = first ? 1 : 0;
  a.inv_batch = inv_batch; a.lr = lr; a.momentum = momentum; a.wd = wd;
  feat_grad_kernel<OWM><<<p.grad_blocks + p.k_blocks, 256, project ? (OWM ? 1 : 2) * p.lds_bytes : 0, st>>>(a);
  MLA_CHECK_LAUNCH("feat_grad_kernel");
  if (!project) return MLA_OK;
  if constexpr (OWM) {
    feat_finish_owm_kernel<<<D, 64 * FEAT_WAVES, p.lds_bytes, st>>>(Pl, w32, w32 + D, ws + p.G, W, buf, D, C, (float)alpha, lr, momentum, wd,
                                                                    first ? 1 : 0);
    MLA_CHECK_LAUNCH("feat_finish_owm_kernel");
  } else {
    feat_rowsq_kernel<<<cdiv(D, 4), 256, 0, st>>>(Pl, w64, w64 + D, w64 + 2 * (size_t)D, D, alpha);
    MLA_CHECK_LAUNCH("feat_rowsq_kernel");
    feat_finish_kernel<<<D, 64 * FEAT_WAVES, p.lds_bytes, st>>>(Pl, w64, w64 + D, w64 + 2 * (size_t)D, ws + p.G, W, buf, D, C, alpha, lr, momentum,
                                                                wd, first ? 1 : 0);
    MLA_CHECK_LAUNCH("feat_finish_kernel");
  }
  return MLA_OK;
}

extern "C" int mla_feature_phase(const float* X, const int64_t* labels, float* W, float* b, float* buf, float* Pl, float* logits,
                                 float* loss, float* ws, int B, int D, int C, float inv_batch, int project, double alpha, float lr,
                                 float momentum, float wd, int first, void* stream) {
  return feature_phase_run<false>("mla_feature_phase", X, labels, W, b, buf, Pl, logits, loss, ws, B, D, C, inv_batch, project, alpha, lr,
                                  momentum, wd, first, stream);
}

extern "C" int mla_feature_phase_owm(const float* X, const int64_t* labels, float* W, float* b, float* buf, float* Pl, float* logits,
                                     float* loss, float* ws, int B, int D, int C, float inv_batch, int project, double alpha, float lr,
                                     float momentum, float wd, int first, void* stream) {
  return feature_phase_run<true>("mla_feature_phase_owm", X, labels, W, b, buf, Pl, logits, loss, ws, B, D, C, inv_batch, project, alpha,
                                 lr, momentum, wd, first, stream);
}

// ---- batch feed from device-resident tables: one workgroup per batch row ---------------------------------------------------------
// The index is clamped to [0, N): the range check belongs to the host, where the index is produced (mla_gather_index_check); the
// kernel never reads outside the tables whatever it is handed.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows2_kernel(const float* __restrict__ T0, const float* __restrict__ T1,
                                                            const int64_t* __restrict__ labels, const int64_t* __restrict__ idx,
                                                            float* __restrict__ out0, float* __restrict__ out1,
                                                            int64_t* __restrict__ out_label, int64_t* __restrict__ out_idx, int N,
                                                            int D) {
  const int b = blockIdx.x;
  int64_t s = idx[b];
  s = s < 0 ? 0 : (s >= N ? (int64_t)N - 1 : s);
  const size_t src = (size_t)s * D, dst = (size_t)b * D;
  if (VEC) {
    const f32x4* a0 = reinterpret_cast<const f32x4*>(T0 + src);
    const f32x4* a1 = reinterpret_cast<const f32x4*>(T1 + src);
    f32x4* o0 = reinterpret_cast<f32x4*>(out0 + dst);
    f32x4* o1 = reinterpret_cast<f32x4*>(out1 + dst);
    for (int j = threadIdx.x; j < (D >> 2); j += 256) {
      o0[j] = a0[j];
      o1[j] = a1[j];
    }
  } else {
    for (int j = threadIdx.x; j < D; j += 256) {
      out0[dst + j] = T0[src + j];
      out1[dst + j] = T1[src + j];
    }
  }
  if (threadIdx.x == 0) {
    out_label[b] = labels[s];
    out_idx[b] = s;
  }
}

extern "C" int mla_gather_index_check(const int64_t* idx_host, int n, int N) { return gather_index_check(idx_host, n, N); }

extern "C" int mla_gather_rows2(const float* T0, const float* T1, const int64_t* labels, const int64_t* idx, float* out0, float* out1,
                                int64_t* out_label, int64_t* out_idx, int N, int D, int B, void* stream) {
  int vec = 0;
  const int rc = gather_rows2_plan(T0, T1, labels, idx, out0, out1, out_label, out_idx, N, D, B, &vec);
  if (rc != MLA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (vec) gather_rows2_kernel<true><<<B, 256, 0, st>>>(T0, T1, labels, idx, out0, out1, out_label, out_idx, N, D);
  else gather_rows2_kernel<false><<<B, 256, 0, st>>>(T0, T1, labels, idx, out0, out1, out_label, out_idx, N, D);
  MLA_CHECK_LAUNCH("gather_rows2_kernel");
  return MLA_OK;
}
