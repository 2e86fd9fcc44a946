// The gated fusion family w_m ~ a_m exp(-beta H_m) (include/mla_hip.h): a non-negative prior per modality, sharpened or softened
// per sample by the entropies H_m of its own class distributions.  beta = 0 is the (normalised) fixed-weight fusion of valid()
// (main.py:647-651), a = 1 and beta = 1 the per-sample form of main.py:65-106 (mla_eval_head mode 1).
//   mla_gate_sweep        every gate (a, beta) of a grid scored on one batch's logits in ONE launch.  Logits and entropies do not
//                         depend on the gate: fusion_sweep_kernel's structure (fusion_sweep.hip) -- one lane per gate, a row tile
//                         staged in LDS, broadcast reads -- with one stage more, a wave per (row, modality) forming H from the
//                         staged row.
//   mla_eval_head_gated   one batch from features to counters under ONE gate: eval_head_kernel (eval_head.hip) with the gate in
//                         place of its modes.  A sibling kernel, so the code object of modes 0 and 1 is what it was.
// Both form their weights with gate_weights (gate_args.h) from entropies formed by gate_row_entropy: a sweep row and an apply call
// with the same gate predict the same class on every row.
#include "gate_args.h"

template <int ROWS>
__global__ __launch_bounds__(SWEEP_LANES) void gate_sweep_kernel(const GateSweepArgs a, const long row_tiles) {
  __shared__ float lg[ROWS][MLA_HEAD_MAXM][MLA_HEAD_MAXC];            // 1.5 KB per row
  __shared__ float ent[ROWS][MLA_HEAD_MAXM];
  __shared__ int lab[ROWS];                                           // the row's label; -1: the row is counted nowhere
  __shared__ int elig[ROWS];                                          // bit k: modality k is present
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, M = a.M, C = a.C;
  const int g = blockIdx.y * SWEEP_LANES + tid;
  const bool live = g < a.G;                                          // dead lanes stage, form entropies and keep the barriers company
  float pr[MLA_HEAD_MAXM] = {0.f, 0.f, 0.f}, beta = 0.f;
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (live && k < M) pr[k] = a.grid[(size_t)g * (M + 1) + k];
  if (live) beta = a.grid[(size_t)g * (M + 1) + M];
  int *const tp = a.tp + (size_t)(live ? g : 0) * C, *const pp = a.pp + (size_t)(live ? g : 0) * C;

  for (long t = blockIdx.x; t < row_tiles; t += gridDim.x) {
    const long r0 = t * ROWS;
    const int rows = a.B - r0 < ROWS ? (int)(a.B - r0) : ROWS;
#pragma unroll
    for (int k = 0; k < MLA_HEAD_MAXM; ++k)
      if (k < M) {
        const float* src = (k == 0 ? a.l[0] : (k == 1 ? a.l[1] : a.l[2])) + (size_t)r0 * C;   // the tile's rows are contiguous
        for (int i = tid; i < rows * C; i += SWEEP_LANES) {
          const int rl = i / C;
          lg[rl][k][i - rl * C] = src[i];
        }
      }
    if (tid < rows) {
      const size_t row = (size_t)r0 + tid;
      const long lab_raw = (long)a.labels[row];
      const int e = eval_present_mask(a.present, row, M);
      const bool bad = eval_bad_label(lab_raw, C) || e == 0;
      lab[tid] = bad ? -1 : (int)lab_raw;
      elig[tid] = e;
      if (!bad && a.num && blockIdx.y == 0) atomicAdd(&a.num[(int)lab_raw], 1);                // once per row, not per gate
    }
    __syncthreads();
    for (int task = wave; task < rows * M; task += SWEEP_LANES / 64) {                         // wave-uniform: one wave per (row, modality)
      const int rl = task / M, k = task - rl * M;
      const float h = gate_row_entropy(head_softmax2(lg[rl][k], C, lane));
      if (lane == 0) {
        ent[rl][k] = h;
        if (a.ent_out && blockIdx.y == 0) a.ent_out[((size_t)r0 + rl) * M + k] = h;
      }
    }
    __syncthreads();
    if (live) {
      for (int rl = 0; rl < rows; ++rl) {
        const int l = lab[rl], e = elig[rl];
        if (l < 0) continue;                                          // never index the tables with a bad label
        float H[MLA_HEAD_MAXM], w[MLA_HEAD_MAXM];
#pragma unroll
        for (int k = 0; k < MLA_HEAD_MAXM; ++k) H[k] = k < M ? ent[rl][k] : 0.f;
        if (!gate_weights(pr, beta, H, e, M, w)) continue;            // nothing the row has carries a share: the pair adds nothing
        const int arg = eval_scan_first_max(C, [&](int c) { return eval_fused_slot(M, w, [&](int k) { return lg[rl][k][c]; }); });
        atomicAdd(&pp[arg], 1);
        if (arg == l) atomicAdd(&tp[l], 1);
      }
    }
    __syncthreads();                                                  // the next tile overwrites what the slower waves still read
  }
}

static int gate_rows = 1;               // the row tile: 1 measured fastest, as in fusion_sweep_kernel

extern "C" int mla_gate_sweep_tile(int rows) {
  if (rows == 1 || rows == 2 || rows == GATE_MAX_ROWS) gate_rows = rows;
  return gate_rows;
}

extern "C" int mla_gate_sweep(const float* l0, const float* l1, const float* l2, const int64_t* labels, const uint8_t* present,
                              const float* grid, int* tp, int* pp, int* num, float* ent_out, int M, int B, int C, int G,
                              void* stream) {
  GateSweepArgs a;
  a.l[0] = l0; a.l[1] = l1; a.l[2] = l2;
  a.labels = labels; a.present = present; a.grid = grid; a.tp = tp; a.pp = pp; a.num = num; a.ent_out = ent_out;
  a.M = M; a.B = B; a.C = C; a.G = G;
  SweepPlan p;
  const int rows = gate_rows;
  MLA_TRY(gate_sweep_plan(&a, rows, &p));
  const dim3 blocks(p.blocks_x, p.blocks_y);
  if (rows == 1) gate_sweep_kernel<1><<<blocks, p.threads, 0, (hipStream_t)stream>>>(a, p.row_tiles);
  else if (rows == 2) gate_sweep_kernel<2><<<blocks, p.threads, 0, (hipStream_t)stream>>>(a, p.row_tiles);
  else gate_sweep_kernel<GATE_MAX_ROWS><<<blocks, p.threads, 0, (hipStream_t)stream>>>(a, p.row_tiles);
  MLA_CHECK_LAUNCH("gate_sweep_kernel");
  return MLA_OK;
}

// ---- mla_eval_head_gated -----------------------------------------------------------------------------------------------------------
// eval_head_kernel's mapping and its first two stages, line for line: one wave per (row, modality), EVAL_ROWS rows per workgroup, the
// logits by head_row_dot + bias (logits_out equals mla_head_logits bit for bit), softmax, entropy and first maximum per wave.  After
// the barrier the row's first wave forms the gate's weights, fuses, takes the fused arg-max and increments the counters.
__global__ __launch_bounds__(64 * MLA_HEAD_MAXM * EVAL_ROWS) void eval_head_gated_kernel(const EvalHeadArgs a, const float beta) {
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
    const float h = gate_row_entropy(sm);
    const int am = eval_first_max2(sm.l0, sm.l1, sm.mx, C, lane);
    if (lane == 0) {
      ent[rl][m] = h;
      arg[rl][m] = am;
    }
  }
  __syncthreads();
  if (!live || m != 0) return;

  // The row's first wave; every lane computes the (wave-uniform) weights.
  const long lab = (long)a.labels[row];
  const int e = eval_present_mask(a.present, (size_t)row, M);
  float H[MLA_HEAD_MAXM], w[MLA_HEAD_MAXM] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k) H[k] = k < M ? ent[rl][k] : 0.f;
  bool bad = eval_bad_label(lab, C) || e == 0;
  if (!bad) bad = !gate_weights(a.alpha, beta, H, e, M, w);           // a pair the sweep leaves out is a bad row here
  if (bad) w[0] = w[1] = w[2] = NAN;

  const float v0 = lane < C ? eval_fused_slot(M, w, [&](int k) { return lg[rl][k][lane]; }) : 0.f;
  const float v1 = lane + 64 < C ? eval_fused_slot(M, w, [&](int k) { return lg[rl][k][lane + 64]; }) : 0.f;
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

extern "C" int mla_eval_head_gated(const float* x0, const float* x1, const float* x2, const float* W, const float* b,
                                   const int64_t* labels, const uint8_t* present, int* counts, float* logits_out, float* fused_out,
                                   float* weights_out, int* pred_out, int M, int B, int D, int C, float prior0, float prior1,
                                   float prior2, float beta, void* stream) {
  EvalHeadArgs a;
  a.x[0] = x0; a.x[1] = x1; a.x[2] = x2;
  a.W = W; a.bias = b; a.labels = labels; a.present = present;
  a.counts = counts; a.logits_out = logits_out; a.fused_out = fused_out; a.weights_out = weights_out; a.pred_out = pred_out;
  a.alpha[0] = prior0; a.alpha[1] = prior1; a.alpha[2] = prior2;
  a.M = M; a.B = B; a.D = D; a.C = C; a.mode = 1;
  EvalPlan p;
  MLA_TRY(eval_head_gated_plan(&a, beta, &p));
  eval_head_gated_kernel<<<p.blocks, p.threads, 0, (hipStream_t)stream>>>(a, beta);
  MLA_CHECK_LAUNCH("eval_head_gated_kernel");
  return MLA_OK;
}
