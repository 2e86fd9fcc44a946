// The head-gradient projection with the scalar denominator of the recursive-least-squares / OWM rule the published one was taken
// from (gs_mode="owm").  Only utils/utils.py:36-40 change:
//
//   k  = Pl r^T                        (D)
//   s  = alpha + r . k                 (scalar; >= alpha when Pl is PSD)
//   Pl <- Pl - k k^T / s               (no renormalisation)
//   G  <- G Pl^T                       (with the updated Pl)
//
// Two launches and no copy (the literal rule, head_gs_sgd.hip: three launches and a device-to-device copy):
//   A. gs_owm_k_kernel       a wave per row of Pl forms k_i in gs_k_kernel's lane / stride order; the same grid copies G into the workspace
//   B. gs_owm_finish_kernel  one workgroup per row i: s (every wave and every workgroup in the same order: the same bits), row i updated,
//                            stored and kept in LDS, then wave w forms G[c][i] for c = w, w + 4, ... from the copy and writes G in place
// fp32 throughout: s >= alpha is well away from zero.  Every sum has one order, there are no atomics, and the only grid dependency is
// the kernel boundary.  The element update Pl[i][j] - (k_i * k_j) / s is symmetric in (i, j): a Pl that starts symmetric stays
// symmetric bit for bit (k_i * (k_j / s) would not be).
#include "common.h"
#include "gs_args.h"

__global__ __launch_bounds__(64 * GS_OWM_WAVES) void gs_owm_k_kernel(const float* __restrict__ Pl, const float* __restrict__ r,
                                                                      const float* __restrict__ G, float* __restrict__ k,
                                                                      float* __restrict__ Gcopy, int D, size_t n_g) {
  const int i = blockIdx.x * GS_OWM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i < D) {
    float s = 0.f;
    for (int j = lane; j < D; j += 64) s += Pl[(size_t)i * D + j] * r[j];
    s = wave_sum(s);
    if (lane == 0) k[i] = s;
  }
  const size_t nthr = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_g; e += nthr) Gcopy[e] = G[e];
}

__global__ __launch_bounds__(64 * GS_OWM_WAVES) void gs_owm_finish_kernel(float* __restrict__ Pl, const float* __restrict__ r,
                                                                           const float* __restrict__ k,
                                                                           const float* __restrict__ Gcopy, float* __restrict__ G,
                                                                           int D, int C, float alpha) {
  extern __shared__ __attribute__((aligned(16))) float row_s[];
  const int i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float t = 0.f;
  for (int j = lane; j < D; j += 64) t += r[j] * k[j];
  const float s = alpha + wave_sum(t);
  const float ki = k[i];
  for (int j = threadIdx.x; j < D; j += 64 * GS_OWM_WAVES) {
    const float v = Pl[(size_t)i * D + j] - (ki * k[j]) / s;
    Pl[(size_t)i * D + j] = v;
    row_s[j] = v;
  }
  __syncthreads();
  for (int c = wave; c < C; c += GS_OWM_WAVES) {
    float g = 0.f;
    for (int j = lane; j < D; j += 64) g += Gcopy[(size_t)c * D + j] * row_s[j];
    g = wave_sum(g);
    if (lane == 0) G[(size_t)c * D + i] = g;
  }
}

extern "C" size_t mla_gs_owm_ws_elems(int D, int C) { return gs_owm_ws_elems(D, C); }

extern "C" int mla_gs_project_owm(float* Pl, const float* r, float* G, int D, int C, float alpha, float* ws, void* stream) {
  GsOwmPlan p;
  const int rc = gs_owm_plan(Pl, r, G, ws, D, C, &p);
  if (rc != MLA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  gs_owm_k_kernel<<<p.k_blocks, 64 * GS_OWM_WAVES, 0, st>>>(Pl, r, G, ws + p.k, ws + p.G, D, (size_t)C * D);
  MLA_CHECK_LAUNCH("gs_owm_k_kernel");
  gs_owm_finish_kernel<<<D, 64 * GS_OWM_WAVES, p.lds_bytes, st>>>(Pl, r, ws + p.k, ws + p.G, G, D, C, alpha);
  MLA_CHECK_LAUNCH("gs_owm_finish_kernel");
  return MLA_OK;
}
