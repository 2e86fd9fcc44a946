// Evaluation metrics beyond accuracy, on the device: a score store filled by one launch per batch (mla_scores_append), average
// precision per head and class without a sort (mla_average_precision) and confusion counts (mla_confusion_count).  The store keeps
// what valid() of the reference forms and drops (main.py:653-657): prediction = softmax(out), pred_a, pred_v.
//
// Average precision of one class with P positives: sklearn's sum over distinct thresholds of (R_n - R_{n-1}) P_n equals
// (1 / P) sum over positives p of TP(>= s_p) / CNT(>= s_p): the k positives of a tie group each contribute the precision at the end
// of their group, together the group's recall step k / P.  Labels are single-label, so a stored row is a positive of exactly one
// class and owns exactly one term.  Both counts are integers; the only floating-point order is the one written in ap_finalize_kernel.
#include "metrics_args.h"

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per (row, head).  Head 0 of a store whose fused logits were never materialised is formed here from the modality rows and
// the weight vector mla_eval_fuse wrote: eval_fused_slot's sum (eval_common.h), the row eval_fuse_kernel took its arg-max of.
__global__ __launch_bounds__(64 * METRICS_WAVES) void scores_append_kernel(const ScoresAppendArgs a) {
  __shared__ float fl[METRICS_WAVES][MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long unit = (long)blockIdx.x * METRICS_WAVES + wave;
  if (unit >= (long)a.B * a.H) return;
  const int r = (int)(unit / a.H), h = (int)(unit - (long)r * a.H);
  const int C = a.C;
  const float* row;
  if (h == 0 && a.weights) {
    const int M = a.H - 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = lane + 64 * k;
      if (c < C) {
        float v = 0.f;             // eval_fused_slot written out: called, the append row came out slower
#pragma unroll
        for (int m = 0; m < MLA_HEAD_MAXM; ++m)
          if (m < M) v += a.weights[m] * a.logits[1 + m][(size_t)r * C + c];
        fl[wave][c] = v;                                              // read back by this lane alone: no barrier
      }
    }
    row = fl[wave];
  } else {
    row = (h == 0 ? a.logits[0] : h == 1 ? a.logits[1] : h == 2 ? a.logits[2] : a.logits[3]) + (size_t)r * C;
  }
  const Softmax2 sm = head_softmax2(row, C, lane);
  const int am = eval_first_max2(sm.l0, sm.l1, sm.mx, C, lane);
  const size_t at = (size_t)a.pos + r;
  float* col = a.scores + (size_t)h * C * a.cap + at;
  if (lane < C) col[(size_t)lane * a.cap] = sm.e0 / sm.s;
  if (lane + 64 < C) col[(size_t)(lane + 64) * a.cap] = sm.e1 / sm.s;
  if (lane != 0) return;
  a.pred[(size_t)h * a.cap + at] = am;
  if (h == 0) {
    const long lab = (long)a.labels[r];
    a.labels_out[at] = lab < INT_MIN || lab > INT_MAX ? -1 : (int)lab; // outside int32 is outside [0, C) too
  }
}

extern "C" int mla_scores_append(const float* l0, const float* l1, const float* l2, const float* l3, const float* weights,
                                 const int64_t* labels, float* scores, int* pred, int* labels_out, int H, int B, int C, int pos,
                                 int cap, void* stream) {
  ScoresAppendArgs a;
  a.logits[0] = l0; a.logits[1] = l1; a.logits[2] = l2; a.logits[3] = l3;
  a.weights = weights; a.labels = labels; a.scores = scores; a.pred = pred; a.labels_out = labels_out;
  a.H = H; a.B = B; a.C = C; a.pos = pos; a.cap = cap;
  MetricsPlan p;
  MLA_TRY(scores_append_plan(&a, &p));
  scores_append_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("scores_append_kernel");
  return MLA_OK;
}

// Terms: one wave per (head, stored row).  ws[h][r] = TP(>= s) / CNT(>= s) at the row's own score in its own class; 0.0 for a row
// whose label is no class or whose score is NaN (x >= NaN holds for no x).
__global__ __launch_bounds__(64 * METRICS_WAVES) void ap_terms_kernel(const AvgPrecisionArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long unit = (long)blockIdx.x * METRICS_WAVES + wave;
  if (unit >= (long)a.N * a.H) return;
  const int h = (int)(unit / a.N), r = (int)(unit - (long)h * a.N);
  double* out = a.ws + (size_t)h * a.cap + r;
  const int c = a.labels[r];
  if (c < 0 || c >= a.C) {
    if (lane == 0) *out = 0.0;
    return;
  }
  const float* col = a.scores + ((size_t)h * a.C + c) * a.cap;
  const float s = col[r];
  int ge = 0, tp = 0;
  for (int n = lane; n < a.N; n += 64) {
    const bool g = col[n] >= s;
    ge += g ? 1 : 0;
    tp += g && a.labels[n] == c ? 1 : 0;
  }
  ge = wave_sum_i(ge);
  tp = wave_sum_i(tp);
  if (lane == 0) *out = ge ? (double)tp / (double)ge : 0.0;
}

// Finalize: one wave per (head, class).  Lane l adds the terms of its rows l, l + 64, ... that belong to the class, in increasing row
// order, then the butterfly of wave_sum_d, then one division.  That order is the definition (tests/metrics_model.py: ap_ordered).
__global__ __launch_bounds__(64 * METRICS_WAVES) void ap_finalize_kernel(const AvgPrecisionArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int unit = blockIdx.x * METRICS_WAVES + wave;
  if (unit >= a.H * a.C) return;
  const int h = unit / a.C, c = unit - h * a.C;
  const double* t = a.ws + (size_t)h * a.cap;
  double acc = 0.0;
  int cnt = 0;
  for (int n = lane; n < a.N; n += 64)
    if (a.labels[n] == c) {
      acc += t[n];
      ++cnt;
    }
  acc = wave_sum_d(acc);
  cnt = wave_sum_i(cnt);
  if (lane != 0) return;
  a.ap[(size_t)h * a.C + c] = cnt ? acc / (double)cnt : (double)NAN;
  if (h == 0) a.npos[c] = cnt;
}

extern "C" size_t mla_metrics_ws_bytes(int cap, int H) { return metrics_ws_bytes(cap, H); }

extern "C" int mla_average_precision(const float* scores, const int* labels, int N, int cap, int H, int C, double* ap, int* npos,
                                     double* ws, void* stream) {
  AvgPrecisionArgs a;
  a.scores = scores; a.labels = labels; a.ap = ap; a.npos = npos; a.ws = ws;
  a.N = N; a.cap = cap; a.H = H; a.C = C;
  MetricsPlan p;
  MLA_TRY(average_precision_plan(&a, &p));
  ap_terms_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("ap_terms_kernel");
  ap_finalize_kernel<<<p.blocks2, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("ap_finalize_kernel");
  return MLA_OK;
}

// conf[h][true][predicted] += 1 for every stored row with a label inside [0, C) -- a row with another label is skipped, as
// eval_fuse_kernel counts it nowhere (not in `num` either) -- and a prediction inside [0, C).
__global__ __launch_bounds__(256) void confusion_kernel(const ConfusionArgs a) {
  const long units = (long)a.N * a.H;
  for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
    const int h = (int)(u / a.N), n = (int)(u - (long)h * a.N);
    const int l = a.labels[n], p = a.pred[(size_t)h * a.cap + n];
    if (l < 0 || l >= a.C || p < 0 || p >= a.C) continue;
    atomicAdd(&a.conf[((size_t)h * a.C + l) * a.C + p], 1);
  }
}

extern "C" int mla_confusion_count(const int* pred, const int* labels, int N, int cap, int H, int C, int* conf, void* stream) {
  ConfusionArgs a;
  a.pred = pred; a.labels = labels; a.conf = conf;
  a.N = N; a.cap = cap; a.H = H; a.C = C;
  MetricsPlan p;
  MLA_TRY(confusion_plan(&a, &p));
  confusion_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a);
  MLA_CHECK_LAUNCH("confusion_kernel");
  return MLA_OK;
}
