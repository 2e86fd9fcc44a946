// Pieces shared by the split-bf16 kernels (conv_igemm_split.hip, conv_patch_split.hip, wgrad_tr_split.hip, stem_split.hip, attention_split.hip):
// fp32 -> three bf16 terms, the product set, and the MFMA / LDS idioms every one of those kernels is built from.
#pragma once
#include "igemm_common.h"

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ds_read_b64_tr_b16, gfx950's transposing LDS read: a 16-lane group reads 4 rows x 16 columns of 16-bit elements (lane 4q + p
// supplies the 8-byte-aligned address of row q, columns 4p .. 4p+3) and lane c of the group receives column c of the 4 rows.
// EXEC must be all ones.
__device__ __forceinline__ s16x4 lds_tr(const unsigned* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p);
}

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {   // low half = bf16(a), high half = bf16(b), RNE
  f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// a - b as ONE v_sub_f32: the SLP vectoriser otherwise pairs the two residual subtractions of split_pair into v_pk_add_f32,
// which costs more issue time beside MFMAs than the two scalar subtractions it replaces (gather-GEMM forward / input gradient:
// -0.5...1 % time in a same-box A/B; weight gradient -3.5 %: there the packing even needs v_mov pairs to line the registers up.
// Residuals by v_dot2c_f32_bf16 (one instruction instead of expand + subtract) measured +4...6 % slower and not bit-identical)
__device__ __forceinline__ float sub_scalar(float a, float b) {
  float r;
  asm("v_sub_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// two fp32 values -> three packed bf16 pairs with x = hi + mid + lo exactly
template <bool NOPK = false>
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned& hi, unsigned& mid, unsigned& lo) {
  hi = cvt_pk_bf16(x0, x1);
  float r0, r1;
  if constexpr (NOPK) {
    r0 = sub_scalar(x0, __uint_as_float(hi << 16));
    r1 = sub_scalar(x1, __uint_as_float(hi & 0xffff0000u));
  } else {
    r0 = x0 - __uint_as_float(hi << 16);
    r1 = x1 - __uint_as_float(hi & 0xffff0000u);
  }
  mid = cvt_pk_bf16(r0, r1);
  if constexpr (NOPK) {
    r0 = sub_scalar(r0, __uint_as_float(mid << 16));
    r1 = sub_scalar(r1, __uint_as_float(mid & 0xffff0000u));
  } else {
    r0 -= __uint_as_float(mid << 16);
    r1 -= __uint_as_float(mid & 0xffff0000u);
  }
  lo = cvt_pk_bf16(r0, r1);
}

__device__ __forceinline__ u32x4 buf_load4u(rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
}

// Products kept, largest first; TERMS = 6 is the fp32-equivalent set (i + j <= 2), 8 adds the 2^-24 terms,
// 3 is the "bf16x3" set (relative error ~2^-16 per product: NOT fp32-equivalent, kept for measurements only).
__device__ constexpr int TERM_A[8] = {0, 0, 1, 1, 0, 2, 1, 2};
__device__ constexpr int TERM_B[8] = {0, 1, 0, 1, 2, 0, 2, 1};

__device__ __forceinline__ bf16x8_t as_bf16x8(bf16x8_t v) { return v; }
__device__ __forceinline__ bf16x8_t as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8_t, v); }

// Helpers for the idioms the split kernels share.  A kernel adopts one only where its generated code stays the same instruction for
// instruction; the sites that keep a sequence written out (the accumulator clears of the gather-GEMM and patch kernels, the staging
// stores of the patch and transposing-read kernels, the MFMA groups on wgrad_tr_split.hip's dword-granular frag() and on the stem
// forward's masked u32x4 fragments) are the ones whose register allocation or schedule moved when routed through here.
__device__ __forceinline__ void zero_acc(f32x16& acc) {
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
}
template <typename T, int N>
__device__ __forceinline__ void zero_acc(T (&acc)[N]) {   // f32x16[N], f32x16[MI][NI]
#pragma unroll
  for (int n = 0; n < N; ++n) zero_acc(acc[n]);
}

// The product group of one 16-deep k-chunk: acc += sum over the first TERMS products of a[TERM_A] * b[TERM_B], planes as
// bf16x8_t or as the u32x4 they were read as.  Product order, then mi, then ni: the summation order the bit-exact tests fix.
// NP = planes held per operand: 3, or 1 with TERMS = 1 (conv_math "bf16": hi * hi alone, one MFMA per fragment pair).
template <int TERMS, typename AT, typename BT, int NP>
__device__ __forceinline__ void split_mma(const AT (&a)[NP], const BT (&b)[NP], f32x16& acc) {
  static_assert(NP == 3 || (NP == 1 && TERMS == 1), "one plane holds the hi * hi product only");
#pragma unroll
  for (int term = 0; term < TERMS; ++term)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[TERM_A[term]]), as_bf16x8(b[TERM_B[term]]), acc, 0, 0, 0);
}
template <int TERMS, int MI, int NI, typename AT, typename BT, int NP>
__device__ __forceinline__ void split_mma(const AT (&a)[NP][MI], const BT (&b)[NP][NI], f32x16 (&acc)[MI][NI]) {
  static_assert(NP == 3 || (NP == 1 && TERMS == 1), "one plane holds the hi * hi product only");
#pragma unroll
  for (int term = 0; term < TERMS; ++term)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[TERM_A[term]][mi]), as_bf16x8(b[TERM_B[term]][ni]), acc[mi][ni], 0, 0, 0);
}

// Four consecutive k of one row -> 8 B in each of the three bf16 planes (`plane` dwords apart); NP = 1: the hi plane alone,
// one conversion per pair and no residuals
template <int NP = 3>
__device__ __forceinline__ void split_store4(unsigned* dst, int plane, f32x4 v) {
  if constexpr (NP == 1) {
    *reinterpret_cast<u32x2*>(dst) = u32x2{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
    return;
  }
  unsigned h0, m0, l0, h1, m1, l1;
  split_pair<true>(v[0], v[1], h0, m0, l0);
  split_pair<true>(v[2], v[3], h1, m1, l1);
  *reinterpret_cast<u32x2*>(dst) = u32x2{h0, h1};
  *reinterpret_cast<u32x2*>(dst + plane) = u32x2{m0, m1};
  *reinterpret_cast<u32x2*>(dst + 2 * plane) = u32x2{l0, l1};
}

// MFMA operand fragments out of an LDS plane image [rows][LR dwords] (one ds_read_b128 each).  Lane (i, h) holds
// k = kk * 16 + 8 h .. + 7 of row / column i; frag_koff is that chunk's dword offset in a row whose swizzle key is swz.
template <int MI, int NI, int NP = 3>
struct SplitFrags { bf16x8_t a[NP][MI], b[NP][NI]; };
__device__ __forceinline__ bf16x8_t lds_frag(const unsigned* p) { return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4*>(p)); }
__device__ __forceinline__ int frag_koff(int kk, int h, int swz) { return ((kk * 2 + h) ^ swz) << 2; }
// Ar / Br: this lane's chunk in plane 0, block 0 of images with BM / BN rows per plane
template <int BM, int BN, int LR, int MI, int NI, int NP>
__device__ __forceinline__ void load_split_frags(const unsigned* Ar, const unsigned* Br, SplitFrags<MI, NI, NP>& f) {
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) f.a[pl][mi] = lds_frag(Ar + (pl * BM + mi * 32) * LR);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) f.b[pl][ni] = lds_frag(Br + (pl * BN + ni * 32) * LR);
  }
}

// The MFMA C / D layout: accumulator element e of lane (i, h) is column i, row acc_row(e) + 4 h of its 32 x 32 block
__device__ __forceinline__ constexpr int acc_row(int e) { return (e & 3) + 8 * (e >> 2); }
