// mla_eval_head: the evaluation of one batch from features to counters in ONE launch (main.py:636-676 with the gating of
// main.py:65-106 applied to each sample's own class distribution, the form the reference's commented-out softmax(dim=1) and
// the method describe; head_gs_sgd.hip's eval_fuse_kernel keeps the published batch-axis form).
//
// One wave per (row, modality), EVAL_ROWS rows per workgroup.  A wave forms its modality's logits with head_row_dot + bias --
// the sum and the order of head_logits_kernel, so logits_out[m] equals mla_head_logits bit for bit -- keeps them in LDS, and
// takes the row's softmax, entropy and first maximum.  After one barrier the row's first wave gates, fuses, takes the fused
// arg-max and increments the counters.  Every float written is a function of its row alone: the only atomics are the integer
// counters, nothing is exchanged between workgroups, and the result does not depend on the batch a row arrives in.
#include "eval_args.h"

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// First slot that holds the row maximum mx (numpy.argmax), a lane holding the slots lane and lane + 64.  A row in which no slot
// equals mx (non-finite logits, outside the contract) answers 0: always inside [0, C).
__device__ __forceinline__ int first_max2(float v0, float v1, float mx, int C, int lane) {
  int i = INT_MAX;
  if (lane + 64 < C && v1 == mx) i = lane + 64;
  if (lane < C && v0 == mx) i = lane;
  i = wave_min_i(i);
  return i < C ? i : 0;
}

__global__ __launch_bounds__(64 * MLA_HEAD_MAXM * EVAL_ROWS) void eval_head_kernel(const EvalHeadArgs a) {
  __shared__ float lg[EVAL_ROWS][MLA_HEAD_MAXM][MLA_HEAD_MAXC];      // 3 KB
  __shared__ float ent[EVAL_ROWS][MLA_HEAD_MAXM];
  __shared__ int arg[EVAL_ROWS][MLA_HEAD_MAXM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rl = wave / a.M, m = wave - rl * a.M;
  const int row = blockIdx.x * EVAL_ROWS + rl;
  const bool live = row < a.B;                                        // dead waves only keep the barriers company
  const int C = a.C, M = a.M;
  if (live) {
    const float* x = (m == 0 ? a.x[0] : (m == 1 ? a.x[1] : a.x[2])) + (size_t)row * a.D;
    float* out = a.logits_out + ((size_t)m * a.B + row) * C;
    for (int c = 0; c < C; ++c) {
      const float s = head_row_dot(x, a.W + (size_t)c * a.D, a.D, lane);
      if (lane == 0) {
        const float v = s + a.bias[c];
        out[c] = v;
        lg[rl][m][c] = v;
      }
    }
  }
  __syncthreads();                                                    // lane 0's logits reach the other lanes of its wave
  if (live) {
    const Softmax2 sm = head_softmax2(lg[rl][m], C, lane);
    float h = 0.f;
    if (a.mode == 1) {
      // H = - sum_c p_c lp_c; a slot whose exp underflowed to 0 contributes its limit 0 (not 0 * -inf), slots past C hold e = 0
      const float t0 = sm.e0 != 0.f ? (sm.e0 / sm.s) * ((sm.l0 - sm.mx) - sm.logs) : 0.f;
      const float t1 = sm.e1 != 0.f ? (sm.e1 / sm.s) * ((sm.l1 - sm.mx) - sm.logs) : 0.f;
      h = 0.f - wave_sum(t0 + t1);
    }
    const int am = first_max2(sm.l0, sm.l1, sm.mx, C, lane);
    if (lane == 0) {
      ent[rl][m] = h;
      arg[rl][m] = am;
    }
  }
  __syncthreads();
  if (!live || m != 0) return;

  // the row's first wave; every lane computes the (wave-uniform) weights
  const long lab = (long)a.labels[row];
  bool el[MLA_HEAD_MAXM];
  int n_el = 0;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) {
    el[k] = k < M && (!a.present || a.present[(size_t)row * M + k] != 0);
    n_el += el[k] ? 1 : 0;
  }
  bool bad = lab < 0 || lab >= C || n_el == 0;
  float w[MLA_HEAD_MAXM] = {0.f, 0.f, 0.f};
  if (a.mode == 1) {                                                  // main.py:72-106 on this row, over the eligible modalities
    float hmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k)
      if (el[k]) hmax = fmaxf(hmax, ent[rl][k]);
    float g[MLA_HEAD_MAXM];
    double sum = 0.0;           // 1 <= g <= 128 (H <= log C): three such floats add exactly in fp64, so the sum has no order
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k) {
      g[k] = el[k] ? expf(hmax - ent[rl][k]) : 0.f;
      sum += (double)g[k];
    }
    const float s = (float)sum;
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = el[k] ? g[k] / s : 0.f;
  } else if (n_el == M) {                                             // main.py:647-651
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = k < M ? a.alpha[k] : 0.f;
  } else {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k)
      if (el[k]) s += a.alpha[k];
    bad = bad || !(s > 0.f);                                          // what is left carries no share of the fusion
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k) w[k] = el[k] ? a.alpha[k] / s : 0.f;
  }
  if (bad) w[0] = w[1] = w[2] = NAN;

  float v0 = 0.f, v1 = 0.f;                                           // fused = sum_m w_m l_m, modalities in order
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (k < M) {
      if (lane < C) v0 += w[k] * lg[rl][k][lane];
      if (lane + 64 < C) v1 += w[k] * lg[rl][k][lane + 64];
    }
  if (a.fused_out) {
    if (lane < C) a.fused_out[(size_t)row * C + lane] = v0;
    if (lane + 64 < C) a.fused_out[(size_t)row * C + lane + 64] = v1;
  }
  const float mx = wave_max(fmaxf(lane < C ? v0 : -INFINITY, lane + 64 < C ? v1 : -INFINITY));
  const int af = first_max2(v0, v1, mx, C, lane);
  if (lane != 0) return;
  if (a.weights_out) {
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k)
      if (k < M) a.weights_out[(size_t)row * M + k] = w[k];
  }
  if (a.pred_out) {
    int* p = a.pred_out + (size_t)row * (1 + M);
    p[0] = bad ? -1 : af;
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k)
      if (k < M) p[1 + k] = bad ? -1 : arg[rl][k];
  }
  if (bad) return;                                                    // counted nowhere; the counters are never indexed with it
  const int l = (int)lab;
  atomicAdd(&a.counts[l], 1);
  if (af == l) atomicAdd(&a.counts[C + l], 1);
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (k < M && arg[rl][k] == l) atomicAdd(&a.counts[C * (2 + k) + l], 1);
}

extern "C" int mla_eval_head(const float* x0, const float* x1, const float* x2, const float* W, const float* b, const int64_t* labels,
                             const uint8_t* present, int* counts, float* logits_out, float* fused_out, float* weights_out,
                             int* pred_out, int M, int B, int D, int C, int mode, float alpha0, float alpha1, float alpha2,
                             void* stream) {
  EvalHeadArgs a;
  a.x[0] = x0; a.x[1] = x1; a.x[2] = x2;
  a.W = W; a.bias = b; a.labels = labels; a.present = present;
  a.counts = counts; a.logits_out = logits_out; a.fused_out = fused_out; a.weights_out = weights_out; a.pred_out = pred_out;
  a.alpha[0] = alpha0; a.alpha[1] = alpha1; a.alpha[2] = alpha2;
  a.M = M; a.B = B; a.D = D; a.C = C; a.mode = mode;
  EvalPlan p;
  const int rc = eval_head_plan(&a, &p);
  if (rc != MLA_OK) return rc;
  eval_head_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("eval_head_kernel");
  return MLA_OK;
}
