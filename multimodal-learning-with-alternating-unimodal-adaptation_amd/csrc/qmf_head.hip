// QMF joint step head (--modulation QMF; main.py:170-268 training, :544-586 validation; utils/utils.py:44-95 History; main.py:108-125
// rank_loss).  Per modality m a Linear head z_m = x_m W_m^T + b_m (audio_fc / visual_fc / txtual_fc), the energy E_m = logsumexp z_m,
// the confidence c_m = E_m / 10, the fused logits out = sum_m c_m z_m (c_m detached), the per-sample cross entropies that feed the
// History, the ranking loss on neighbouring samples of the batch, and every gradient.
//
// Latency-bound (64 x 512 x 6): four launches for the training call, one for the forward.  Wave-per-class dot products with 64-lane
// shuffle reductions, no atomics, one writer per History entry, every sum in a fixed order (bitwise reproducible from run to run).
#include "head_common.h"

#define QH_CHUNKS 256         // lo / hi partials per modality (one per thread of the kernel that finishes the reduction)

namespace {

struct QmfPtrs {
  const float* x[MLA_HEAD_MAXM];   // (B, D) features of modality m
  const float* W[MLA_HEAD_MAXM];   // (C, D) head weight
  const float* b[MLA_HEAD_MAXM];   // (C) head bias
  float* dW[MLA_HEAD_MAXM];
  float* db[MLA_HEAD_MAXM];
  float* dx[MLA_HEAD_MAXM];        // (B, D) feature gradients
};

// (a) One workgroup (4 waves) per sample.  Wave w forms z_m[c] for c = w, w + 4, ... of every modality; wave m then forms E_m, c_m
// and (TRAIN) softmax p_m and the per-sample CE l_m, and makes the History write when this sample is the LAST of the batch that
// carries its index (numpy's buffered `a[idx] += v`: one writer per entry, no race); all threads form out = sum_m c_m z_m; wave 0
// (TRAIN) the softmax / CE of `out` and its share of dlogits, (p_out - onehot) * inv_batch.
// A label outside [0, C) or an index outside [0, n_data): NaN losses for the sample, no History write.
template <bool TRAIN>
__global__ __launch_bounds__(256) void qmf_head_fwd_kernel(const QmfPtrs p, const int64_t* __restrict__ labels,
                                                            const int64_t* __restrict__ idx, double* __restrict__ correctness,
                                                            double* __restrict__ confidence, int n_data, float* __restrict__ z,
                                                            float* __restrict__ out, float* __restrict__ conf,
                                                            float* __restrict__ ell, float* __restrict__ prob,
                                                            float* __restrict__ dfused, float* __restrict__ rowcml, int M, int B,
                                                            int D, int C, float inv_batch) {
  __shared__ float zl[MLA_HEAD_MAXM][MLA_HEAD_MAXC];
  __shared__ float ol[MLA_HEAD_MAXC];
  __shared__ float cl[MLA_HEAD_MAXM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  for (int m = 0; m < M; ++m) {
    const float* x = p.x[m] + (size_t)row * D;
    for (int c = wave; c < C; c += 4) {
      const float* w = p.W[m] + (size_t)c * D;
      const float s = head_row_dot(x, w, D, lane) + p.b[m][c];
      if (lane == 0) {
        z[((size_t)m * B + row) * C + c] = s;
        zl[m][c] = s;
      }
    }
  }
  __syncthreads();
  bool ok = true;
  int lab = 0;
  long id = 0;
  if (TRAIN) {
    const long lab_raw = (long)labels[row];
    id = (long)idx[row];
    ok = lab_raw >= 0 && lab_raw < C && id >= 0 && id < n_data;
    lab = ok ? (int)lab_raw : 0;
  }
  if (wave < M) {
    const int m = wave;
    // head_softmax2's expressions, written out: through the helper the LDS address of zl[m][.] is formed another way and the
    // kernel's instruction stream changes
    const float l0 = lane < C ? zl[m][lane] : -INFINITY;
    const float l1 = lane + 64 < C ? zl[m][lane + 64] : -INFINITY;
    const float mx = wave_max(fmaxf(l0, l1));
    const float e0 = lane < C ? expf(l0 - mx) : 0.f, e1 = lane + 64 < C ? expf(l1 - mx) : 0.f;
    const float s = wave_sum(e0 + e1);
    const float logs = logf(s);
    const float E = mx + logs;
    const float cm = E / 10.f;                                          // main.py:245-246
    if (lane == 0) {
      conf[(size_t)m * B + row] = cm;
      cl[m] = cm;
    }
    if (TRAIN) {
      const float lm = ok ? head_ce_loss(logs, mx, zl[m][lab]) : NAN;         // CrossEntropyLoss(reduction='none'), main.py:255-256
      if (lane < C) prob[((size_t)m * B + row) * C + lane] = e0 / s;
      if (lane + 64 < C) prob[((size_t)m * B + row) * C + lane + 64] = e1 / s;
      // last occurrence of this index inside the batch writes (utils/utils.py:57-58)
      float later = 0.f;
      for (int k = row + 1 + lane; k < B; k += 64) later += ((long)idx[k] == id) ? 1.f : 0.f;
      later = wave_sum(later);
      if (lane == 0) {
        ell[(size_t)m * B + row] = lm;
        if (ok && later == 0.f) {
          correctness[(size_t)m * n_data + id] += (double)lm;
          confidence[(size_t)m * n_data + id] = (double)cm;
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float o = 0.f;
    for (int m = 0; m < M; ++m) o += cl[m] * zl[m][c];                  // main.py:249 (confidences detached)
    ol[c] = o;
    out[(size_t)row * C + c] = o;
  }
  if (!TRAIN) return;
  __syncthreads();
  if (wave == 0) {
    const Softmax2 q = head_softmax2(ol, C, lane);
    if (lane == 0) rowcml[row] = ok ? head_ce_loss(q.logs, q.mx, ol[lab]) * inv_batch : NAN;
    if (lane < C) dfused[(size_t)row * C + lane] = ok ? head_ce_grad(q.e0, q.s, lane == lab, inv_batch) : 0.f;
    if (lane + 64 < C) dfused[(size_t)row * C + lane + 64] = ok ? head_ce_grad(q.e1, q.s, lane + 64 == lab, inv_batch) : 0.f;
  }
}

// (b) grid (chunks, M): block (k, m) reduces entries k * 256 + t, stride chunks * 256, of modality m's correctness to one (lo, hi)
// pair (utils/utils.py:67-69: min / max over ALL n_data entries).  min / max do not depend on the order.
__global__ __launch_bounds__(256) void qmf_lohi_kernel(const double* __restrict__ correctness, double* __restrict__ part, int n_data,
                                                        int chunks) {
  __shared__ double slo[4], shi[4];
  const int m = blockIdx.y;
  const double* c = correctness + (size_t)m * n_data;
  double lo = INFINITY, hi = -INFINITY;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n_data; k += (long)chunks * 256) {
    const double v = c[k];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  lo = wave_min_d(lo);
  hi = wave_max_d(hi);
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)m * QH_CHUNKS + blockIdx.x) * 2;
    o[0] = fmin(fmin(slo[0], slo[1]), fmin(slo[2], slo[3]));
    o[1] = fmax(fmax(shi[0], shi[1]), fmax(shi[2], shi[3]));
  }
}

// (c) One workgroup per sample i.  Finishes lo / hi, then for the pairs (i, i + 1) and (i - 1, i) (indices mod B) of every modality:
// n = (correctness - lo) / (hi - lo) in fp64, t = sign(n_i - n_j), mg = |n_i - n_j|, r = c_j + mg / (t ? t : 1), the hinge
// max(0, t (c_i - r)) (main.py:108-125; MarginRankingLoss with target -t).  With a = [t (c_i - r) > 0] the confidence c_m[i] collects
// q = (t_i a_i - t_{i-1} a_{i-1}) * inv_batch (both operands of the pair carry gradient), and
//   dz_m[i] = (p_m - onehot) inv_batch + w_cml c_m[i] dfused[i] + w_crl q p_m / 10,      dX_m[i] = dz_m[i] W_m.
__global__ __launch_bounds__(256) void qmf_head_rank_kernel(const QmfPtrs p, const int64_t* __restrict__ labels,
                                                             const int64_t* __restrict__ idx, const double* __restrict__ correctness,
                                                             const double* __restrict__ part, int n_data, int chunks,
                                                             const float* __restrict__ conf, const float* __restrict__ prob,
                                                             const float* __restrict__ dfused, float* __restrict__ dz,
                                                             float* __restrict__ target, float* __restrict__ margin,
                                                             float* __restrict__ rowrank, int M, int B, int D, int C, float w_cml,
                                                             float w_crl, float inv_batch) {
  __shared__ double slo[MLA_HEAD_MAXM][4], shi[MLA_HEAD_MAXM][4];
  __shared__ float ta[MLA_HEAD_MAXM][2];                // t * a of the pairs (i, i + 1) and (i - 1, i)
  __shared__ float dzl[MLA_HEAD_MAXM][MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  for (int m = 0; m < M; ++m) {
    double lo = INFINITY, hi = -INFINITY;
    if ((int)threadIdx.x < chunks) {
      lo = part[((size_t)m * QH_CHUNKS + threadIdx.x) * 2];
      hi = part[((size_t)m * QH_CHUNKS + threadIdx.x) * 2 + 1];
    }
    lo = wave_min_d(lo);
    hi = wave_max_d(hi);
    if (lane == 0) {
      slo[m][wave] = lo;
      shi[m][wave] = hi;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * M) {
    const int m = threadIdx.x >> 1, which = threadIdx.x & 1;
    const int i = which == 0 ? row : (row + B - 1) % B;
    const int j = (i + 1) % B;
    const double lo = fmin(fmin(slo[m][0], slo[m][1]), fmin(slo[m][2], slo[m][3]));
    const double hi = fmax(fmax(shi[m][0], shi[m][1]), fmax(shi[m][2], shi[m][3]));
    const long ii = (long)idx[i], ij = (long)idx[j];
    const long li = (long)labels[i], lj = (long)labels[j];
    const bool ok = ii >= 0 && ii < n_data && ij >= 0 && ij < n_data && li >= 0 && li < C && lj >= 0 && lj < C;
    float t = 0.f, mg = NAN, hinge = NAN, act = 0.f;
    if (ok) {
      const double ni = (correctness[(size_t)m * n_data + ii] - lo) / (hi - lo);       // utils/utils.py:66-71
      const double nj = (correctness[(size_t)m * n_data + ij] - lo) / (hi - lo);
      t = ni > nj ? 1.f : (ni < nj ? -1.f : 0.f);                                      // :86-89
      mg = (float)fabs(ni - nj);                                                        // :92-93
      const float ci = conf[(size_t)m * B + i], cj = conf[(size_t)m * B + j];
      const float r = cj + mg / (t == 0.f ? 1.f : t);                                   // main.py:116-118
      const float v = t * (ci - r);
      act = v > 0.f ? 1.f : 0.f;
      hinge = v > 0.f ? v : (v != v ? v : 0.f);                                         // a NaN margin (hi == lo) stays NaN
    }
    ta[m][which] = t * act;
    if (which == 0) {
      target[(size_t)m * B + row] = t;
      margin[(size_t)m * B + row] = mg;
      rowrank[(size_t)m * B + row] = hinge * inv_batch;
    }
  }
  __syncthreads();
  const long lab_raw = (long)labels[row], id = (long)idx[row];
  const bool ok = lab_raw >= 0 && lab_raw < C && id >= 0 && id < n_data;
  for (int k = threadIdx.x; k < M * C; k += 256) {
    const int m = k / C, c = k - m * C;
    const float pm = prob[((size_t)m * B + row) * C + c];
    const float q = (ta[m][0] - ta[m][1]) * inv_batch;
    float g = (pm - (c == (int)lab_raw ? 1.f : 0.f)) * inv_batch + w_cml * conf[(size_t)m * B + row] * dfused[(size_t)row * C + c] +
              w_crl * q * pm / 10.f;
    if (!ok) g = 0.f;
    dzl[m][c] = g;
    dz[((size_t)m * B + row) * C + c] = g;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < M * D; k += 256) {
    const int m = k / D, d = k - m * D;
    const float* w = p.W[m] + d;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += dzl[m][c] * w[(size_t)c * D];
    p.dx[m][(size_t)row * D + d] = a;
  }
}

// (d) grid (ceil(D / 256) * M, C): dW_m[c][d] = sum_rows dz_m[row][c] x_m[row][d] (rows in order); the first block of a modality
// also db_m[c]; block (0, 0) the losses [L, CE_0 .. CE_{M-1}, rank_0 .. rank_{M-1}, CE(out)] with
// L = w_cml CE(out) + sum_m CE(z_m) + w_crl sum_m rank_m (main.py:265-268 / :203, 229).
__global__ __launch_bounds__(256) void qmf_head_dw_kernel(const QmfPtrs p, const float* __restrict__ dz, const float* __restrict__ ell,
                                                           const float* __restrict__ rowrank, const float* __restrict__ rowcml,
                                                           float* __restrict__ losses, int M, int B, int D, int C, float w_cml,
                                                           float w_crl, float inv_batch) {
  const int per = (D + 255) / 256;
  const int m = blockIdx.x / per, c = blockIdx.y;
  const int d = (blockIdx.x - m * per) * 256 + threadIdx.x;
  const float* g = dz + (size_t)m * B * C + c;
  if (d < D) {
    const float* x = p.x[m] + d;
    float a = 0.f;
    for (int r = 0; r < B; ++r) a += g[(size_t)r * C] * x[(size_t)r * D];
    p.dW[m][(size_t)c * D + d] = a;
  }
  if (blockIdx.x == m * per && threadIdx.x < 64) {
    const float a = head_col_sum(g, B, C, 0, threadIdx.x);
    if (threadIdx.x == 0) p.db[m][c] = a;
    if (blockIdx.x == 0 && c == 0) {
      float clf = 0.f, crl = 0.f;
      for (int k = 0; k < M; ++k) {
        float l = 0.f, rk = 0.f;
        for (int r = threadIdx.x; r < B; r += 64) {
          l += ell[(size_t)k * B + r];
          rk += rowrank[(size_t)k * B + r];
        }
        l = wave_sum(l) * inv_batch;
        rk = wave_sum(rk);
        clf += l;
        crl += rk;
        if (threadIdx.x == 0) {
          losses[1 + k] = l;
          losses[1 + M + k] = rk;
        }
      }
      const float cml = head_col_sum(rowcml, B, 1, 0, threadIdx.x);
      if (threadIdx.x == 0) {
        losses[1 + 2 * M] = cml;
        losses[0] = w_cml * cml + clf + w_crl * crl;
      }
    }
  }
}

QmfPtrs make_ptrs(const float* const* x, const float* const* W, const float* const* b, float* const* dW, float* const* db,
                  float* const* dx, int M) {
  QmfPtrs p;
  for (int m = 0; m < MLA_HEAD_MAXM; ++m) {
    const bool on = m < M;
    p.x[m] = on ? x[m] : nullptr;
    p.W[m] = on ? W[m] : nullptr;
    p.b[m] = on ? b[m] : nullptr;
    p.dW[m] = on && dW ? dW[m] : nullptr;
    p.db[m] = on && db ? db[m] : nullptr;
    p.dx[m] = on && dx ? dx[m] : nullptr;
  }
  return p;
}

bool all_set(const void* const* q, int M) {
  for (int m = 0; m < M; ++m)
    if (!q[m]) return false;
  return true;
}

int lohi_chunks(int n_data) { return n_data < QH_CHUNKS * 256 ? cdiv(n_data, 256) : QH_CHUNKS; }

}  // namespace

// floats: the fp64 lo / hi partials first (the workspace is 8-byte aligned), then prob, dz (M B C each), dfused (B C), rowcml (B),
// rowrank (M B)
extern "C" size_t mla_qmf_head_ws_elems(int B, int C, int M) {
  return (size_t)4 * MLA_HEAD_MAXM * QH_CHUNKS + (size_t)2 * M * B * C + (size_t)B * C + (size_t)B + (size_t)M * B;
}

extern "C" int mla_qmf_head_fwd_bwd(const float* x0, const float* x1, const float* x2, const float* W0, const float* W1,
                                    const float* W2, const float* b0, const float* b1, const float* b2, const int64_t* labels,
                                    const int64_t* idx, double* correctness, double* confidence, int n_data, float* z, float* out,
                                    float* conf, float* ell, float* target, float* margin, float* losses, float* dW0, float* dW1,
                                    float* dW2, float* db0, float* db1, float* db2, float* dx0, float* dx1, float* dx2, float* ws,
                                    int M, int B, int D, int C, float w_cml, float w_crl, float inv_batch, void* stream) {
  MLA_REQUIRE(M == 2 || M == 3, "mla_qmf_head_fwd_bwd: M must be 2 or 3 (got %d)", M);
  const float *x[3] = {x0, x1, x2}, *W[3] = {W0, W1, W2}, *b[3] = {b0, b1, b2};
  float *dW[3] = {dW0, dW1, dW2}, *db[3] = {db0, db1, db2}, *dx[3] = {dx0, dx1, dx2};
  MLA_REQUIRE(all_set((const void* const*)x, M) && all_set((const void* const*)W, M) && all_set((const void* const*)b, M) &&
                  all_set((const void* const*)dW, M) && all_set((const void* const*)db, M) && all_set((const void* const*)dx, M) &&
                  labels && idx && correctness && confidence && z && out && conf && ell && target && margin && losses && ws,
              "mla_qmf_head_fwd_bwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0 && C <= MLA_HEAD_MAXC && n_data > 0,
              "mla_qmf_head_fwd_bwd: need B, D, n_data > 0 and 0 < C <= %d (got B %d D %d C %d n_data %d)", MLA_HEAD_MAXC, B, D, C, n_data);
  MLA_REQUIRE(((uintptr_t)ws & 7) == 0, "mla_qmf_head_fwd_bwd: the workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const QmfPtrs p = make_ptrs(x, W, b, dW, db, dx, M);
  double* part = (double*)ws;
  float* prob = ws + (size_t)4 * MLA_HEAD_MAXM * QH_CHUNKS;
  float* dz = prob + (size_t)M * B * C;
  float* dfused = dz + (size_t)M * B * C;
  float* rowcml = dfused + (size_t)B * C;
  float* rowrank = rowcml + B;
  const int chunks = lohi_chunks(n_data);
  qmf_head_fwd_kernel<true><<<B, 256, 0, st>>>(p, labels, idx, correctness, confidence, n_data, z, out, conf, ell, prob, dfused,
                                                rowcml, M, B, D, C, inv_batch);
  MLA_CHECK_LAUNCH("qmf_head_fwd_kernel<train>");
  qmf_lohi_kernel<<<dim3(chunks, M), 256, 0, st>>>(correctness, part, n_data, chunks);
  MLA_CHECK_LAUNCH("qmf_lohi_kernel");
  qmf_head_rank_kernel<<<B, 256, 0, st>>>(p, labels, idx, correctness, part, n_data, chunks, conf, prob, dfused, dz, target, margin,
                                          rowrank, M, B, D, C, w_cml, w_crl, inv_batch);
  MLA_CHECK_LAUNCH("qmf_head_rank_kernel");
  qmf_head_dw_kernel<<<dim3(cdiv(D, 256) * M, C), 256, 0, st>>>(p, dz, ell, rowrank, rowcml, losses, M, B, D, C, w_cml, w_crl,
                                                                 inv_batch);
  MLA_CHECK_LAUNCH("qmf_head_dw_kernel");
  return MLA_OK;
}

extern "C" int mla_qmf_head_fwd(const float* x0, const float* x1, const float* x2, const float* W0, const float* W1, const float* W2,
                                const float* b0, const float* b1, const float* b2, float* z, float* out, float* conf, int M, int B,
                                int D, int C, void* stream) {
  MLA_REQUIRE(M == 2 || M == 3, "mla_qmf_head_fwd: M must be 2 or 3 (got %d)", M);
  const float *x[3] = {x0, x1, x2}, *W[3] = {W0, W1, W2}, *b[3] = {b0, b1, b2};
  MLA_REQUIRE(all_set((const void* const*)x, M) && all_set((const void* const*)W, M) && all_set((const void* const*)b, M) && z && out &&
                  conf,
              "mla_qmf_head_fwd: null pointer");
  MLA_REQUIRE(B > 0 && D > 0 && C > 0 && C <= MLA_HEAD_MAXC, "mla_qmf_head_fwd: need B, D > 0 and 0 < C <= %d (got %d)", MLA_HEAD_MAXC, C);
  const QmfPtrs p = make_ptrs(x, W, b, nullptr, nullptr, nullptr, M);
  qmf_head_fwd_kernel<false><<<B, 256, 0, (hipStream_t)stream>>>(p, nullptr, nullptr, nullptr, nullptr, 0, z, out, conf, nullptr,
                                                                 nullptr, nullptr, nullptr, M, B, D, C, 0.f);
  MLA_CHECK_LAUNCH("qmf_head_fwd_kernel");
  return MLA_OK;
}
