// torch.optim.Adam (amsgrad=False, maximize=False), single-tensor rule, over one flat range per launch (main.py:736-747 --cav_opti;
// main.py:31 --optimizer).  Memory-bound: 4 reads + 3 writes of 4 B per element.  The body runs on 16-byte loads / stores from the
// first 16-byte boundary of p on; the <= 3 elements before it and the <= 3 after the last whole float4 are scalar.  p, m and v of a
// range normally share their misalignment (slices flat[o:o+n] of buffers allocated alike); when they do not, the whole range runs
// scalar, and a gradient that alone is off takes four dword loads per float4 of the others.
#include "adam_args.h"
#include "common.h"

struct AdamK {
  float step_size, beta1, beta2, bc2_sqrt, eps, wd;
};

// The arithmetic in torch's order: grad.add(param, alpha=wd); exp_avg.lerp_(grad, 1 - beta1); exp_avg_sq.mul_(beta2).addcmul_(grad,
// grad, value=1 - beta2); denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps); param.addcdiv_(exp_avg, denom, -step_size).
// The multiply-adds are written as fused ones, not left to the contraction flags: g + wd p cancels when a gradient element
// nearly equals -wd p, and only the single rounding keeps the small result's relative error at an ulp (ATen's vectorised CPU
// kernels fuse it too).
template <typename T>
__device__ __forceinline__ T splat(float x) {
  if constexpr (sizeof(T) == sizeof(float)) return x;
  else return T{x, x, x, x};
}

template <typename T>
__device__ __forceinline__ void adam_update(T& p, T g, T& m, T& v, const AdamK k) {
  g = __builtin_elementwise_fma(p, splat<T>(k.wd), g);
  m = __builtin_elementwise_fma(g - m, splat<T>(1.0f - k.beta1), m);
  v = __builtin_elementwise_fma(g * g, splat<T>(1.0f - k.beta2), v * k.beta2);
  const T den = __builtin_elementwise_sqrt(v) / k.bc2_sqrt + k.eps;
  p = p - (m / den) * k.step_size;
}

template <bool GVEC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n, size_t head, size_t n4, const AdamK k) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + head);
  f32x4* m4 = reinterpret_cast<f32x4*>(m + head);
  f32x4* v4 = reinterpret_cast<f32x4*>(v + head);
  for (size_t i = tid; i < n4; i += nthr) {
    f32x4 pv = p4[i], mv = m4[i], vv = v4[i], gv = {0.f, 0.f, 0.f, 0.f};
    if (g) {
      if constexpr (GVEC) {
        gv = reinterpret_cast<const f32x4*>(g + head)[i];
      } else {
        const float* gs = g + head + 4 * i;
        gv = f32x4{gs[0], gs[1], gs[2], gs[3]};
      }
    }
    adam_update(pv, gv, mv, vv, k);
    m4[i] = mv;
    v4[i] = vv;
    p4[i] = pv;
  }
  // everything outside the float4 body: [0, head) and [head + 4 n4, n) (at most 6 elements; all of n on the scalar launch)
  const size_t rest = n - 4 * n4;
  for (size_t r = tid; r < rest; r += nthr) {
    const size_t i = r < head ? r : r + 4 * n4;
    float pv = p[i], mv = m[i], vv = v[i];
    adam_update(pv, g ? g[i] : 0.f, mv, vv, k);
    m[i] = mv;
    v[i] = vv;
    p[i] = pv;
  }
}

extern "C" int mla_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                             float wd, int step, void* stream) {
  AdamPlan pl;
  const int rc = adam_plan(p, g, m, v, n, lr, beta1, beta2, step, &pl);
  if (rc != MLA_OK) return rc;
  const AdamK k = {pl.step_size, beta1, beta2, pl.bc2_sqrt, eps, wd};
  const size_t work = pl.vec ? pl.n4 : n;                   // threads' worth of grid-stride work
  size_t blocks = (work + 255) / 256;
  const size_t cap = (size_t)mla_cu_count() * 8;            // 8 workgroups of 256 per CU; the rest is the grid-stride loop
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  if (pl.gvec)
    adam_kernel<true><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, pl.head, pl.n4, k);
  else
    adam_kernel<false><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, pl.head, pl.n4, k);
  MLA_CHECK_LAUNCH("adam_kernel");
  return MLA_OK;
}
