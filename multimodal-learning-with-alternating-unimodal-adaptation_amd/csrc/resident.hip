// The HBM-resident CREMA-D feed, gfx950: the whole decoded dataset (uint8 frames, fp32 fbanks, labels) sits on the device and a
// batch is three launches over the epoch's order vector, with no host copy of anything the kernels read:
//
//   resident_draw_kernel      one thread per (batch slot j, frame slot t): i = order[pos + j], row i * T + t of the frame table
//                             (offset, H, W) -> one mla_frames_resample descriptor row (offset, H, W, top, left, h, w, flip) in
//                             `desc`; train: RandomResizedCrop(scale (0.08, 1), ratio (3/4, 4/3)).get_params and
//                             RandomHorizontalFlip drawn from Philox4x32-10 in fp64 (layout and arithmetic: resident_args.h);
//                             eval: the whole frame.  Also label_out[j] = labels[i], idx_out[j] = i.
//   resident_resample_kernel  frames_common.h's <bilinear, 8-column> body over `desc`: crop, Pillow's bilinear resize, flip, LUT,
//                             straight out of the resident buffer.  Its LDS plan is the worst case over every crop the draw can
//                             make (mla_resident_plan, once, on the host copy of the frame table), so no descriptor is read back.
//   resident_gather_kernel    rows order[pos + j] of the fp32 spectrogram table -> spec_out, 16-byte accesses.
//
// The kernels trust nothing they read from device tables further than the host could check it: an order entry is clamped to
// [0, N), a table row that does not lie inside the frame buffer becomes the 1x1 frame at offset 0, a drawn box lies inside its frame
// by construction, and the body's min(rows, rows_cap) keeps the staged rows inside LDS.  No atomics; a frame's pixels depend on
// (seed, epoch, dataset index, frame slot) and the frame alone.
#include "common.h"
#include "frames_common.h"
#include "philox.h"
#include "resident_args.h"

// torchvision RandomResizedCrop.get_params + the central-crop fallback of frames.sample_crop, then the flip: row[3..7]
__device__ __forceinline__ void res_draw(int64_t H, int64_t W, uint64_t key, uint64_t index, int t, int64_t* __restrict__ row) {
#pragma clang fp contract(off)
  const double area = (double)(H * W);
  int64_t top = 0, left = 0, h = 0, w = 0;
  bool found = false;
  uint32_t r[4];
  for (int k = 0; k < RES_TRIES && !found; ++k) {
    philox4x32(res_counter(t, k), index, key, r);
    const double u = (double)r[0] * 0x1p-32, v = (double)r[1] * 0x1p-32;
    const double target = area * (RES_SCALE_LO + RES_SCALE_SPAN * u);
    const double aspect = exp(RES_L0 + (RES_L1 - RES_L0) * v);
    const double dw = rint(sqrt(target * aspect)), dh = rint(sqrt(target / aspect));
    if (dw > 0.0 && dw <= (double)W && dh > 0.0 && dh <= (double)H) {
      w = (int64_t)dw;
      h = (int64_t)dh;
      top = (int64_t)(((uint64_t)r[2] * (uint64_t)(H - h + 1)) >> 32);
      left = (int64_t)(((uint64_t)r[3] * (uint64_t)(W - w + 1)) >> 32);
      found = true;
    }
  }
  if (!found) {
    const double in_ratio = (double)W / (double)H;
    w = W;
    h = H;
    if (in_ratio < RES_RATIO_LO) h = (int64_t)rint((double)W / RES_RATIO_LO);
    else if (in_ratio > RES_RATIO_HI) w = (int64_t)rint((double)H * RES_RATIO_HI);
    h = h < 1 ? 1 : (h > H ? H : h);               // both hold already: W / 0.75 < H and H * 4 / 3 < W in their branches
    w = w < 1 ? 1 : (w > W ? W : w);
    top = (H - h) / 2;
    left = (W - w) / 2;
  }
  philox4x32(res_counter(t, RES_FLIP_SLOT), index, key, r);
  row[3] = top;
  row[4] = left;
  row[5] = h;
  row[6] = w;
  row[7] = r[0] < 0x80000000u ? 1 : 0;
}

__global__ __launch_bounds__(RES_DRAW_THREADS) void resident_draw_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ labels,
                                                                          const int64_t* __restrict__ order, int64_t frames_bytes, int N,
                                                                          int T, int pos, int b, uint64_t key, int train,
                                                                          int64_t* __restrict__ desc, int64_t* __restrict__ label_out,
                                                                          int64_t* __restrict__ idx_out) {
  const int g = blockIdx.x * RES_DRAW_THREADS + threadIdx.x;
  if (g >= b * T) return;
  const int j = g / T, t = g - j * T;
  int64_t i = order[pos + j];
  i = i < 0 ? 0 : (i >= N ? N - 1 : i);
  const int64_t* src = table + ((size_t)i * T + t) * RES_TABLE_COLS;
  int64_t off = src[0], H = src[1], W = src[2];
  if (H <= 0 || W <= 0 || H > FR_DIM_MAX || W > FR_DIM_MAX || off < 0 || H * W * 3 > frames_bytes || off > frames_bytes - H * W * 3) {
    off = 0;
    H = W = 1;
  }
  int64_t* row = desc + (size_t)g * RES_DESC_COLS;
  row[0] = off;
  row[1] = H;
  row[2] = W;
  if (train) {
    res_draw(H, W, key, (uint64_t)i, t, row);
  } else {
    row[3] = 0;
    row[4] = 0;
    row[5] = H;
    row[6] = W;
    row[7] = 0;
  }
  if (t == 0) {
    label_out[j] = labels[i];
    idx_out[j] = i;
  }
}

__global__ __launch_bounds__(FR_THREADS) void resident_resample_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                        const float* __restrict__ lut, float* __restrict__ out, int T,
                                                                        int OH, int OW, int band, int rows_cap, int kh, int kv) {
  fr_body<FR_BILINEAR, RES_DESC_COLS, false>(src, desc, lut, out, nullptr, nullptr, nullptr, T, OH, OW, band, rows_cap, kh, kv);
}

// grid (RES_SPEC_ROW / 4 / (threads * units), b): a workgroup moves threads * units consecutive 16-byte units of one row
__global__ __launch_bounds__(RES_GATHER_THREADS) void resident_gather_kernel(const f32x4* __restrict__ spec, const int64_t* __restrict__ order,
                                                                              int N, int pos, f32x4* __restrict__ out) {
  const int j = blockIdx.y;
  int64_t i = order[pos + j];
  i = i < 0 ? 0 : (i >= N ? N - 1 : i);
  const size_t base = (size_t)blockIdx.x * (RES_GATHER_THREADS * RES_GATHER_UNITS) + threadIdx.x;
  const f32x4* s = spec + (size_t)i * (RES_SPEC_ROW / 4) + base;
  f32x4* o = out + (size_t)j * (RES_SPEC_ROW / 4) + base;
  f32x4 v[RES_GATHER_UNITS];
#pragma unroll
  for (int q = 0; q < RES_GATHER_UNITS; ++q) v[q] = s[q * RES_GATHER_THREADS];
#pragma unroll
  for (int q = 0; q < RES_GATHER_UNITS; ++q) o[q * RES_GATHER_THREADS] = v[q];
}
static_assert((RES_SPEC_ROW / 4) % (RES_GATHER_THREADS * RES_GATHER_UNITS) == 0, "a spectrogram row is a whole number of workgroups");

extern "C" int mla_resident_plan(const int64_t* table_host, int64_t rows, int T, size_t frames_bytes, int out_h, int out_w, int train,
                                 int* plan5) {
  MLA_REQUIRE(plan5, "mla_resident_plan: null plan");
  FramePlan p;
  const int rc = res_plan(table_host, rows, T, frames_bytes, out_h, out_w, train, &p);
  if (rc != MLA_OK) return rc;
  plan5[0] = p.band;
  plan5[1] = p.rows_cap;
  plan5[2] = p.kh;
  plan5[3] = p.kv;
  plan5[4] = (int)p.lds;
  return MLA_OK;
}

extern "C" int mla_resident_batch(const uint8_t* frames, size_t frames_bytes, const int64_t* table, const float* spec_table,
                                  const int64_t* labels, const int64_t* order, int N, int T, int pos, int b, uint64_t seed, uint64_t epoch,
                                  int train, const int* plan5, const float* lut, int64_t* desc_out, float* image_out, float* spec_out,
                                  int64_t* label_out, int64_t* idx_out, int out_h, int out_w, void* stream) {
  FramePlan plan;
  const int rc = res_batch_check(frames, frames_bytes, table, spec_table, labels, order, N, T, pos, b, seed, epoch, plan5, lut, desc_out,
                                 image_out, spec_out, label_out, idx_out, out_h, out_w, &plan);
  if (rc != MLA_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(resident_draw_kernel, dim3((unsigned)cdiv((long)b * T, RES_DRAW_THREADS)), dim3(RES_DRAW_THREADS), 0, st, table, labels,
                     order, (int64_t)frames_bytes, N, T, pos, b, res_key(seed, epoch), train, desc_out, label_out, idx_out);
  MLA_CHECK_LAUNCH("mla_resident_batch (draw)");
  hipLaunchKernelGGL(resident_resample_kernel, dim3((unsigned)cdiv(out_h, plan.band), (unsigned)(b * T)), dim3(FR_THREADS), plan.lds, st,
                     frames, desc_out, lut, image_out, T, out_h, out_w, plan.band, plan.rows_cap, plan.kh, plan.kv);
  MLA_CHECK_LAUNCH("mla_resident_batch (resample)");
  if (spec_table) {
    hipLaunchKernelGGL(resident_gather_kernel, dim3(RES_SPEC_ROW / 4 / (RES_GATHER_THREADS * RES_GATHER_UNITS), (unsigned)b),
                       dim3(RES_GATHER_THREADS), 0, st, reinterpret_cast<const f32x4*>(spec_table), order, N, pos,
                       reinterpret_cast<f32x4*>(spec_out));
    MLA_CHECK_LAUNCH("mla_resident_batch (gather)");
  }
  return MLA_OK;
}
