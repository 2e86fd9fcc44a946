// Evaluation path (main.py:486-679 `valid`, gs_flag branch 622-651), two forms from the same features to the same counter layout:
//   the published chain   M mla_head_logits launches + one mla_eval_fuse: fixed or entropy-gated fusion (main.py:65-106; SURVEY Q9:
//                         the "entropy" is taken over softmax(dim=0), i.e. over the BATCH axis, and summed over the whole tensor ->
//                         one scalar weight per modality per batch), arg-max and the per-class counters of main.py:659-676 -- on
//                         the device, one workgroup, instead of a per-sample .cpu() loop;
//   mla_eval_head         one batch from features to counters in ONE launch, with the gating of main.py:65-106 applied to each
//                         sample's own class distribution, the form the reference's commented-out softmax(dim=1) and the method
//                         describe.
// The arg-max, fusion and bad-row rules of both are eval_common.h's.
#include "eval_args.h"

// ---- the published chain -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_logits_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ logits, int B,
                                                           int D, int C) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const float* x = X + (size_t)row * D;
  for (int c = 0; c < C; ++c) {
    const float s = head_row_dot(x, W + (size_t)c * D, D, lane);
    if (lane == 0) logits[(size_t)row * C + c] = s + bias[c];
  }
}

extern "C" int mla_head_logits(const float* X, const float* W, const float* b, float* logits, int B, int D, int C, void* stream) {
  MLA_REQUIRE(X && W && b && logits && B > 0 && D > 0 && C > 0, "mla_head_logits: bad argument");
  head_logits_kernel<<<cdiv(B, 4), 256, 0, (hipStream_t)stream>>>(X, W, b, logits, B, D, C);
  MLA_CHECK_LAUNCH("head_logits_kernel");
  return MLA_OK;
}

// counts layout (int32, accumulated across calls): [0..C) num per class, then for k = 0 (fused), 1..M (modalities):
// [C*(1+k) .. C*(2+k)) correct per class.  weights_out[M]: the fusion weights used for this batch.
__global__ __launch_bounds__(256) void eval_fuse_kernel(const EvalFuseArgs a, const int64_t* __restrict__ labels,
                                                         int* __restrict__ counts, float* __restrict__ weights_out) {
  __shared__ float ent[MLA_HEAD_MAXM];
  __shared__ float wgt[MLA_HEAD_MAXM];
  __shared__ float colpart[256];
  const int tid = threadIdx.x;
  if (a.dynamic) {
    // entropy_m = - sum_{rows, cols} p log p, p = softmax over ROWS (dim=0) of out_m   (main.py:65-70)
    for (int m = 0; m < a.M; ++m) {
      float acc = 0.f;
      for (int c = tid; c < a.C; c += 256) {           // one column per thread
        float mx = -INFINITY;
        for (int r = 0; r < a.B; ++r) mx = fmaxf(mx, a.out[m][(size_t)r * a.C + c]);
        float s = 0.f;
        for (int r = 0; r < a.B; ++r) s += expf(a.out[m][(size_t)r * a.C + c] - mx);
        const float ls = logf(s);
        for (int r = 0; r < a.B; ++r) {
          const float lp = a.out[m][(size_t)r * a.C + c] - mx - ls;   // log softmax
          acc -= expf(lp) * lp;
        }
      }
      colpart[tid] = acc;
      __syncthreads();
      if (tid == 0) {
        float e = 0.f;
        for (int k = 0; k < 256; ++k) e += colpart[k];
        ent[m] = e;
      }
      __syncthreads();
    }
    if (tid == 0) {                                    // main.py:72-106
      float mx = ent[0];
      for (int m = 1; m < a.M; ++m) mx = fmaxf(mx, ent[m]);
      float sum = 0.f;
      for (int m = 0; m < a.M; ++m) {
        wgt[m] = expf(mx - ent[m]);
        sum += wgt[m];
      }
      for (int m = 0; m < a.M; ++m) wgt[m] /= sum;
    }
  } else if (tid < a.M) {
    wgt[tid] = a.alpha[tid];                           // main.py:647-651
  }
  __syncthreads();
  if (tid < a.M && weights_out) weights_out[tid] = wgt[tid];
  __syncthreads();                                     // a bad label's NaN (below, any wave) lands after thread 0's weights_out[0]
  for (int r = tid; r < a.B; r += 256) {               // one sample per thread
    const long lab_raw = (long)labels[r];
    if (eval_bad_label(lab_raw, a.C)) {                // poison the weights instead
      if (weights_out) weights_out[0] = NAN;
      continue;
    }
    const int lab = (int)lab_raw;
    const size_t at = (size_t)r * a.C;
    atomicAdd(&counts[lab], 1);
    const int arg = eval_scan_first_max(a.C, [&](int c) { return eval_fused_slot(a.M, wgt, [&](int m) { return a.out[m][at + c]; }); });
    if (arg == lab) atomicAdd(&counts[a.C * 1 + lab], 1);
    for (int m = 0; m < a.M; ++m)
      if (eval_scan_first_max(a.C, [&](int c) { return a.out[m][at + c]; }) == lab) atomicAdd(&counts[a.C * (2 + m) + lab], 1);
  }
}

extern "C" int mla_eval_fuse(const float* out0, const float* out1, const float* out2, const int64_t* labels, int* counts,
                             float* weights_out, int M, int B, int C, int dynamic, float alpha0, float alpha1, float alpha2,
                             void* stream) {
  EvalFuseArgs a;
  a.out[0] = out0; a.out[1] = out1; a.out[2] = out2;
  a.alpha[0] = alpha0; a.alpha[1] = alpha1; a.alpha[2] = alpha2;
  a.M = M; a.B = B; a.C = C; a.dynamic = dynamic;
  EvalPlan p;
  MLA_TRY(eval_fuse_plan(&a, labels, counts, &p));
  eval_fuse_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a, labels, counts, weights_out);
  MLA_CHECK_LAUNCH("eval_fuse_kernel");
  return MLA_OK;
}

// ---- mla_eval_head ---------------------------------------------------------------------------------------------------------------
// One wave per (row, modality), EVAL_ROWS rows per workgroup.  A wave forms its modality's logits with head_row_dot + bias --
// the sum and the order of head_logits_kernel, so logits_out[m] equals mla_head_logits bit for bit -- keeps them in LDS, and
// takes the row's softmax, entropy and first maximum.  After one barrier the row's first wave gates, fuses, takes the fused
// arg-max and increments the counters.  Every float written is a function of its row alone: the only atomics are the integer
// counters, nothing is exchanged between workgroups, and the result does not depend on the batch a row arrives in.
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
    const int am = eval_first_max2(sm.l0, sm.l1, sm.mx, C, lane);
    if (lane == 0) {
      ent[rl][m] = h;
      arg[rl][m] = am;
    }
  }
  __syncthreads();
  if (!live || m != 0) return;

  // The row's first wave; every lane computes the (wave-uniform) weights.
  // eval_present_mask / eval_fixed_weights / eval_fused_slot written out: called, they cost this kernel 4.7 %.
  // Only the cross-kernel tests (tests/test_sweep_gpu.py against mla_fusion_sweep) tie the mode-0 copy to eval_fixed_weights.
  const long lab = (long)a.labels[row];
  bool el[MLA_HEAD_MAXM];
  int n_el = 0;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) {
    el[k] = k < M && (!a.present || a.present[(size_t)row * M + k] != 0);
    n_el += el[k] ? 1 : 0;
  }
  bool bad = eval_bad_label(lab, C) || n_el == 0;
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
  } else if (n_el == M) {                                             // eval_fixed_weights: main.py:647-651
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

  float v0 = 0.f, v1 = 0.f;                                           // eval_fused_slot, both slots in one pass over the modalities
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
  const int af = eval_first_max2(v0, v1, mx, C, lane);
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
  if (bad) return;
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
  MLA_TRY(eval_head_plan(&a, &p));
  eval_head_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("eval_head_kernel");
  return MLA_OK;
}
