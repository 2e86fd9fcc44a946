// Modal3Dataset's missing-modality masks (dataset/dataset.py:794-801; IEMOCAP, --modal3), gfx950.  The reference multiplies each
// sample's spectrogram, image, token ids and padding mask by that sample's 0/1 mask entry:
//
//   spectrogram * m[0];  image * m[1];  tokenizer * m[2];  padding_mask * m[2]
//
// Here the batcher loads nothing for an absent modality and runs the image kernels over the P images the batch does have, into a
// compact (P, 3, S, S) buffer.  This one launch finishes the batch: image_out[b] = image_compact[slot[b]] or zeros, and the
// spectrogram, token and padding-mask rows of absent modalities are overwritten with zeros in place (rows of present modalities
// are not touched).  The kernel SELECTS, it never multiplies: the staged row of an absent modality is whatever the pinned ring
// held before (NaN, Inf, anything), and NaN * 0 is NaN.  The zeros written have every bit clear, so +0.0 where the reference's
// x * 0 gives -0.0 for negative x: equal values (torch.equal holds), different sign bit.
//
// Pure bandwidth: a present image moves 2 x 12 S^2 bytes, everything else is written only.  blockIdx.y is the sample, so the four
// presence tests are uniform over a workgroup; a thread moves one 16-byte unit per turn of a grid-stride loop over the sample's
// image | spectrogram | token | padding-mask units.  No atomics, no LDS.
#include "common.h"
#include "modal3_args.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// host (modal3_plan): every range a whole number of 16-byte units from a 16-byte aligned base, slots a permutation of 0..P-1
__global__ __launch_bounds__(MODAL3_THREADS) void modal3_assemble_kernel(const u32x4* __restrict__ image_compact,
                                                                          u32x4* __restrict__ spec, u32x4* __restrict__ token,
                                                                          u32x4* __restrict__ pm, const int64_t* __restrict__ mdesc,
                                                                          u32x4* __restrict__ image_out, const Modal3Plan p) {
  const int b = blockIdx.y;
  const int64_t* d = mdesc + (size_t)b * MODAL3_DESC;
  const bool audio = d[0] != 0, image = d[1] != 0, text = d[2] != 0;
  const u32x4* src = image_compact + (size_t)(image ? d[3] : 0) * p.image;
  u32x4* img = image_out + (size_t)b * p.image;
  u32x4* sp = spec + (size_t)b * p.spec;
  u32x4* tk = token + (size_t)b * p.token;
  u32x4* pk = pm + (size_t)b * p.pm;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const int end_spec = p.image + p.spec, end_token = end_spec + p.token;
  // absent everywhere but the image: only the image units hold work
  const int n = (audio && text) ? p.image : p.total;
  const int stride = gridDim.x * MODAL3_THREADS;
  for (int u = blockIdx.x * MODAL3_THREADS + threadIdx.x; u < n; u += stride) {
    if (u < p.image) {
      img[u] = image ? src[u] : zero;
    } else if (u < end_spec) {
      if (!audio) sp[u - p.image] = zero;
    } else if (u < end_token) {
      if (!text) tk[u - end_spec] = zero;
    } else {
      if (!text) pk[u - end_token] = zero;
    }
  }
}

extern "C" int mla_modal3_assemble_check(const int64_t* mdesc_host, int B, int P, int S, int TF, int L) {
  Modal3Plan p;
  const int rc = modal3_shape_plan(B, S, TF, L, &p);
  return rc != MLA_OK ? rc : modal3_table_check(mdesc_host, B, P);
}

extern "C" int mla_modal3_assemble(const float* image_compact, float* spec, int64_t* token, float* pm, const int64_t* mdesc,
                                   const int64_t* mdesc_host, float* image_out, int B, int P, int S, int TF, int L, void* stream) {
  Modal3Plan p;
  const int rc = modal3_plan(image_compact, spec, token, pm, mdesc, mdesc_host, image_out, B, P, S, TF, L, &p);
  if (rc != MLA_OK) return rc;
  hipLaunchKernelGGL(modal3_assemble_kernel, dim3((unsigned)p.blocks_x, (unsigned)B), dim3(MODAL3_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const u32x4*>(image_compact), reinterpret_cast<u32x4*>(spec), reinterpret_cast<u32x4*>(token),
                     reinterpret_cast<u32x4*>(pm), mdesc, reinterpret_cast<u32x4*>(image_out), p);
  MLA_CHECK_LAUNCH("mla_modal3_assemble");
  return MLA_OK;
}
