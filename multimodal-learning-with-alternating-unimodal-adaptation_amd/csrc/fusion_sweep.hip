// mla_fusion_sweep: the fixed-weight fusion of valid() (main.py:647-651) scored at every point of a grid of fusion weights in ONE
// launch.  The per-modality logits do not depend on the fusion weights, so an evaluation pass that already holds them can score
// G candidate weightings for the few flops after the head instead of G passes through the encoders.
//
// One lane per grid point, its M weights in registers; a workgroup owns SWEEP_LANES grid points (blockIdx.y) and walks row tiles of
// SWEEP_ROWS rows (blockIdx.x, striding).  A tile's logits, labels and eligibility masks are staged in LDS once; every lane then
// reads the same address (a broadcast, no bank conflict).  The class scan, the fused sum and the renormalisation over what a row has
// are eval_common.h's, the ones eval_fuse_kernel and eval_head_kernel (eval_head.hip) call, so a grid point that equals an
// evaluator's alphas predicts what that evaluator predicts, bit for bit.  No cross-lane operation, integer atomics only.
#include "sweep_args.h"

__global__ __launch_bounds__(SWEEP_LANES) void fusion_sweep_kernel(const SweepArgs a, const long row_tiles) {
  __shared__ float lg[SWEEP_ROWS][MLA_HEAD_MAXM][MLA_HEAD_MAXC];      // 1.5 KB
  __shared__ int lab[SWEEP_ROWS];                                     // the row's label; -1: the row is counted nowhere
  __shared__ int elig[SWEEP_ROWS];                                    // bit k: modality k is present
  const int tid = threadIdx.x, M = a.M, C = a.C;
  const int g = blockIdx.y * SWEEP_LANES + tid;
  const bool live = g < a.G;                                          // dead lanes stage and keep the barriers company
  float al[MLA_HEAD_MAXM] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < MLA_HEAD_MAXM; ++k)
    if (live && k < M) al[k] = a.grid[(size_t)g * M + k];
  int *const tp = a.tp + (size_t)(live ? g : 0) * C, *const pp = a.pp + (size_t)(live ? g : 0) * C;

  for (long t = blockIdx.x; t < row_tiles; t += gridDim.x) {
    const long r0 = t * SWEEP_ROWS;
    const int rows = a.B - r0 < SWEEP_ROWS ? (int)(a.B - r0) : SWEEP_ROWS;
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
      if (!bad && a.num && blockIdx.y == 0) atomicAdd(&a.num[(int)lab_raw], 1);                // once per row, not per grid point
    }
    __syncthreads();
    if (live) {
      for (int rl = 0; rl < rows; ++rl) {
        const int l = lab[rl], e = elig[rl];
        if (l < 0) continue;                                          // never index the tables with a bad label
        float w[MLA_HEAD_MAXM];
        if (!eval_fixed_weights(al, e, M, w)) continue;               // what is left carries no share: the pair adds nothing
        const int arg = eval_scan_first_max(C, [&](int c) { return eval_fused_slot(M, w, [&](int k) { return lg[rl][k][c]; }); });
        atomicAdd(&pp[arg], 1);
        if (arg == l) atomicAdd(&tp[l], 1);
      }
    }
    __syncthreads();                                                  // the next tile overwrites what the slower waves still read
  }
}

extern "C" int mla_fusion_sweep(const float* l0, const float* l1, const float* l2, const int64_t* labels, const uint8_t* present,
                                const float* grid, int* tp, int* pp, int* num, int M, int B, int C, int G, void* stream) {
  SweepArgs a;
  a.l[0] = l0; a.l[1] = l1; a.l[2] = l2;
  a.labels = labels; a.present = present; a.grid = grid; a.tp = tp; a.pp = pp; a.num = num;
  a.M = M; a.B = B; a.C = C; a.G = G;
  SweepPlan p;
  MLA_TRY(fusion_sweep_plan(&a, &p));
  fusion_sweep_kernel<<<dim3(p.blocks_x, p.blocks_y), p.threads, 0, (hipStream_t)stream>>>(a, p.row_tiles);
  MLA_CHECK_LAUNCH("fusion_sweep_kernel");
  return MLA_OK;
}
