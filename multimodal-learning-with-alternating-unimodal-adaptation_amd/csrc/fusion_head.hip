// The conventional-fusion heads of the joint (non --gs_flag) step, models/fusion_modules.py of the reference:
//   SumFusion    (:5-13)    out = fc_x(x) + fc_y(y);  out_a = x Wx^T + s bx, out_v = y Wy^T + s by with s = 1 in training
//                           (main.py:292-295) and 0.5 in evaluation (main.py:610-614)
//   FiLM         (:38-67)   gamma | beta = fc(film);  z = gamma * t + beta;  out = fc_out(z)
//   GatedFusion  (:70-98)   hx = fc_x(x), hy = fc_y(y);  z = sigmoid(hx) * hy (x_gate) or hx * sigmoid(hy);  out = fc_out(z)
// each with nn.CrossEntropyLoss (main.py:305) and every gradient.
//
// Latency-bound at the step's shapes (64 x 512 / 768, C <= 128), like the concat head: fp32 throughout, wave dot products with 64-lane
// shuffle reductions, no atomics, every sum in a fixed order (bitwise reproducible from run to run).  Three kernels:
//   fusion_hidden_kernel   the hidden Linear layers (FiLM: fc; gated: fc_x and fc_y in one launch)
//   fusion_row_kernel      one workgroup per sample: z, the logits, softmax / CE / dlogits, dz = dlogits Wout and the gradient at the
//                          hidden outputs (FiLM also d t)
//   fusion_grad_kernel     every Linear layer's dW, db and input gradient in one launch (FusionJobs, fusion_args.h), and the loss sums
// sum: row + grad (2 launches); FiLM / gated: hidden + row + grad (3).
#include "fusion_args.h"
#include "head_common.h"

namespace {

enum { SUM = 0, FILM = 1, GATED = 2 };
enum { FWD = 0, TRAIN = 1, BWD = 2 };

struct HiddenJobs {
  const float* x[2];
  const float* W[2];
  const float* b[2];
  float* h[2];
  int N[2];
};

// grid (ceil(max N / 4), row split, jobs): wave w of block (i, j, k) forms h_k[r][4 i + w] = x_k[r] . W_k[4 i + w] + b_k[4 i + w] for
// the rows r = j, j + gridDim.y, ...
__global__ __launch_bounds__(256) void fusion_hidden_kernel(const HiddenJobs p, int B, int D) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.z;
  const int N = p.N[k];
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  const float* w = p.W[k] + (size_t)n * D;
  const float bn = p.b[k][n];
  for (int r = blockIdx.y; r < B; r += gridDim.y) {
    const float s = head_row_dot(p.x[k] + (size_t)r * D, w, D, lane);
    if (lane == 0) p.h[k][(size_t)r * N + n] = s + bn;
  }
}

struct RowArgs {
  const float *x, *y;            // SUM: the two features.  FILM: y = t, the feature that is modulated.  GATED: unused
  const float *Wa, *ba;          // SUM: fc_x.  FILM / GATED: fc_out
  const float *Wb, *bb;          // SUM: fc_y
  const float *h0, *h1;          // FILM: h0 = (gamma | beta) (B, 2 D).  GATED: hx, hy (B, D)
  float* z;                      // FILM / GATED: (B, D), written by FWD / TRAIN, not touched by BWD
  const int64_t* labels;         // TRAIN
  const float* dl_in;            // BWD: the given d out (B, C)
  float *out, *out_a, *out_v;    // FWD / TRAIN; out_a / out_v SUM only
  float *dlogits, *rowloss;      // TRAIN, BWD: ws
  float* dh;                     // FILM: d(gamma | beta) (B, 2 D); GATED: dhx (B, D) then dhy (B, D)
  float* dt;                     // FILM: d t (B, D)
  int B, D, C, x_gate;
  float inv_batch, bias_scale, scale;
};

// 1 / (1 + exp(-h)): exactly 0.5 at h = 0, 0 where expf overflows (h <= -89), 1 where expf(-h) < 2^-24 (h >= 17)
__device__ __forceinline__ float fusion_sigmoid(float h) { return 1.f / (1.f + expf(-h)); }

template <int METHOD, int MODE>
__global__ __launch_bounds__(256) void fusion_row_kernel(const RowArgs p) {
  __shared__ float zs[METHOD == SUM ? 1 : FUSION_MAXD];
  __shared__ float lg[MLA_HEAD_MAXC];
  __shared__ float lgm[2][MLA_HEAD_MAXC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  const int B = p.B, D = p.D, C = p.C;
  if (MODE != BWD) {
    if (METHOD != SUM) {
      for (int d = threadIdx.x; d < D; d += 256) {
        float z;
        if (METHOD == FILM) {
          const float gamma = p.h0[(size_t)row * 2 * D + d], beta = p.h0[(size_t)row * 2 * D + D + d];
          z = gamma * p.y[(size_t)row * D + d] + beta;                          // fusion_modules.py:64
        } else {
          const float hx = p.h0[(size_t)row * D + d], hy = p.h1[(size_t)row * D + d];
          z = p.x_gate ? fusion_sigmoid(hx) * hy : hx * fusion_sigmoid(hy);     // :92-96
        }
        zs[d] = z;
        p.z[(size_t)row * D + d] = z;
      }
      __syncthreads();
    }
    for (int c = wave; c < C; c += 4) {
      float o;
      if (METHOD == SUM) {
        const float sx = head_row_dot(p.x + (size_t)row * D, p.Wa + (size_t)c * D, D, lane);
        const float sy = head_row_dot(p.y + (size_t)row * D, p.Wb + (size_t)c * D, D, lane);
        o = (sx + p.ba[c]) + (sy + p.bb[c]);                                    // fc_x(x) + fc_y(y), :12
        const float oa = sx + p.ba[c] * p.bias_scale, ov = sy + p.bb[c] * p.bias_scale;
        if (lane == 0) {
          p.out_a[(size_t)row * C + c] = oa;
          p.out_v[(size_t)row * C + c] = ov;
          lgm[0][c] = oa;
          lgm[1][c] = ov;
        }
      } else {
        o = head_row_dot(zs, p.Wa + (size_t)c * D, D, lane) + p.ba[c];
      }
      if (lane == 0) {
        p.out[(size_t)row * C + c] = o;
        lg[c] = o;
      }
    }
    if (MODE == FWD) return;
    __syncthreads();
    const long lab_raw = (long)p.labels[row];
    const bool lab_ok = lab_raw >= 0 && lab_raw < C;    // out of range: NaN loss, zero dlogits (the head family's policy)
    const int lab = lab_ok ? (int)lab_raw : 0;
    if (wave == 0 || (METHOD == SUM && wave <= 2)) {
      // wave 0: the trained logits `out`; SUM, waves 1 and 2: out_a / out_v (loss value only, main.py:308-309)
      const float* l = wave == 0 ? lg : lgm[wave - 1];
      const Softmax2 q = head_softmax2(l, C, lane);
      if (lane == 0) p.rowloss[(size_t)wave * B + row] = lab_ok ? head_ce_loss(q.logs, q.mx, l[lab]) * p.inv_batch : NAN;
      if (wave == 0) {
        __builtin_amdgcn_wave_barrier();              // every lane has read lg before it is overwritten with dlogits
        const float d0 = lab_ok ? head_ce_grad(q.e0, q.s, lane == lab, p.inv_batch) : 0.f;
        const float d1 = lab_ok ? head_ce_grad(q.e1, q.s, lane + 64 == lab, p.inv_batch) : 0.f;
        if (lane < C) {
          lg[lane] = d0;
          p.dlogits[(size_t)row * C + lane] = d0;
        }
        if (lane + 64 < C) {
          lg[lane + 64] = d1;
          p.dlogits[(size_t)row * C + lane + 64] = d1;
        }
      }
    }
    __syncthreads();
    if (METHOD == SUM) return;                        // dX, dY: input gradients of the gradient launch
  } else {
    for (int c = threadIdx.x; c < C; c += 256) {
      const float d = p.dl_in[(size_t)row * C + c] * p.scale;
      lg[c] = d;
      p.dlogits[(size_t)row * C + c] = d;
    }
    if (METHOD == SUM) return;
    __syncthreads();
  }
  // dz[d] = sum_c dlogits[c] Wout[c][d] (classes in order), then through the fusion to the hidden outputs
  for (int d = threadIdx.x; d < D; d += 256) {
    float dz = 0.f;
    for (int c = 0; c < C; ++c) dz += lg[c] * p.Wa[(size_t)c * D + d];
    if (METHOD == FILM) {
      const float gamma = p.h0[(size_t)row * 2 * D + d];
      const float t = p.y[(size_t)row * D + d];
      p.dh[(size_t)row * 2 * D + d] = dz * t;                                   // d gamma
      p.dh[(size_t)row * 2 * D + D + d] = dz;                                   // d beta
      p.dt[(size_t)row * D + d] = dz * gamma;
    } else {
      const float hx = p.h0[(size_t)row * D + d], hy = p.h1[(size_t)row * D + d];
      const float g = fusion_sigmoid(p.x_gate ? hx : hy);
      const float dgate = (dz * (p.x_gate ? hy : hx)) * (g * (1.f - g));        // through the sigmoid
      const float dlin = dz * g;                                                // the ungated side
      p.dh[(size_t)row * D + d] = p.x_gate ? dgate : dlin;                      // dhx
      p.dh[((size_t)B + row) * D + d] = p.x_gate ? dlin : dgate;                // dhy
    }
  }
}

// Block b of job j (FusionJob, fusion_args.h): a dW block (n, 256 columns): dW[n][k] = sum_rows g[r][n] in[r][k] (rows in order), the
// first block of n also db[n] = sum_r g[r][n]; or a din block (row, 256 columns): din[r][k] = sum_n g[r][n] W[n][k] (n in order).
// With `rowloss`, block 0 also sums the nloss loss rows.
__global__ __launch_bounds__(256) void fusion_grad_kernel(const FusionJobs js, const float* __restrict__ rowloss,
                                                           float* __restrict__ losses, int nloss, int B) {
  int ji = 0;
  while (ji + 1 < js.n && (int)blockIdx.x >= js.job[ji + 1].first) ++ji;
  const FusionJob& j = js.job[ji];
  const int b = blockIdx.x - j.first;
  const int N = j.N, K = j.K;
  if (b < j.w_blocks) {
    const int n = b / j.kchunks, k = (b - n * j.kchunks) * 256 + threadIdx.x;
    if (k < K) {
      float a = 0.f;
      for (int r = 0; r < B; ++r) a += j.g[(size_t)r * N + n] * j.in[(size_t)r * K + k];
      j.dW[(size_t)n * K + k] = a;
    }
    if (b == n * j.kchunks && threadIdx.x < 64) {
      const float a = head_col_sum(j.g, B, N, n, threadIdx.x);
      if (threadIdx.x == 0) j.db[n] = a;
    }
  } else {
    const int bb = b - j.w_blocks;
    const int r = bb / j.kchunks, k = (bb - r * j.kchunks) * 256 + threadIdx.x;
    if (k < K) {
      float a = 0.f;
      for (int n = 0; n < N; ++n) a += j.g[(size_t)r * N + n] * j.W[(size_t)n * K + k];
      j.din[(size_t)r * K + k] = a;
    }
  }
  if (blockIdx.x == 0 && rowloss && threadIdx.x < 64) {
    for (int i = 0; i < nloss; ++i) {
      const float l = head_col_sum(rowloss + (size_t)i * B, B, 1, 0, threadIdx.x);
      if (threadIdx.x == 0) losses[i] = l;
    }
  }
}

int launch_hidden(const HiddenJobs& h, int jobs, int B, int D, hipStream_t st) {
  const int nmax = jobs == 2 && h.N[1] > h.N[0] ? h.N[1] : h.N[0];
  fusion_hidden_kernel<<<dim3(cdiv(nmax, 4), B < 8 ? B : 8, jobs), 256, 0, st>>>(h, B, D);
  MLA_CHECK_LAUNCH("fusion_hidden_kernel");
  return MLA_OK;
}

template <int METHOD, int MODE>
int launch_row(const RowArgs& a, hipStream_t st) {
  fusion_row_kernel<METHOD, MODE><<<a.B, 256, 0, st>>>(a);
  MLA_CHECK_LAUNCH("fusion_row_kernel");
  return MLA_OK;
}

int launch_grad(const FusionJobs& js, const float* rowloss, float* losses, int nloss, int B, hipStream_t st) {
  fusion_grad_kernel<<<js.blocks, 256, 0, st>>>(js, rowloss, losses, nloss, B);
  MLA_CHECK_LAUNCH("fusion_grad_kernel");
  return MLA_OK;
}

#define FUSION_PTRS(who, ...)                                              \
  do {                                                                     \
    const void* const ptrs__[] = {__VA_ARGS__};                            \
    MLA_TRY(fusion_check_ptrs(who, ptrs__, (int)(sizeof(ptrs__) / sizeof(ptrs__[0])))); \
  } while (0)

RowArgs row_args(int B, int D, int C) {
  RowArgs a = {};
  a.B = B; a.D = D; a.C = C;
  a.x_gate = 1;
  a.bias_scale = 1.f;
  a.scale = 1.f;
  return a;
}

}  // namespace

extern "C" size_t mla_fusion_ws_elems(int B, int D, int C) { return fusion_ws_elems(B, D, C); }

// ---- sum ----------------------------------------------------------------------------------------------------------------------------
static int sum_grads(const float* x, const float* y, const float* Wx, const float* Wy, const float* dl, float* dWx, float* dbx, float* dWy,
                     float* dby, float* dX, float* dY, const float* rowloss, float* losses, int B, int D, int C, hipStream_t st) {
  FusionJobs js;
  fusion_jobs_init(&js);
  MLA_TRY(fusion_jobs_add(&js, dl, x, Wx, dWx, dbx, dX, B, C, D));
  MLA_TRY(fusion_jobs_add(&js, dl, y, Wy, dWy, dby, dY, B, C, D));
  return launch_grad(js, rowloss, losses, FUSION_NLOSS, B, st);
}

extern "C" int mla_fusion_sum_ce_fwd_bwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                                         const int64_t* labels, float* out, float* out_a, float* out_v, float* losses, float* dWx,
                                         float* dbx, float* dWy, float* dby, float* dX, float* dY, float* ws, int B, int D, int C,
                                         float inv_batch, float bias_scale, void* stream) {
  const char* who = "mla_fusion_sum_ce_fwd_bwd";
  FUSION_PTRS(who, x, y, Wx, bx, Wy, by, out, out_a, out_v, losses, dWx, dbx, dWy, dby, dX, dY, ws);
  MLA_TRY(fusion_check_labels(who, labels));
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  RowArgs a = row_args(B, D, C);
  a.x = x; a.y = y; a.Wa = Wx; a.ba = bx; a.Wb = Wy; a.bb = by; a.labels = labels;
  a.out = out; a.out_a = out_a; a.out_v = out_v; a.dlogits = ws + w.dlogits; a.rowloss = ws + w.rowloss;
  a.inv_batch = inv_batch; a.bias_scale = bias_scale;
  MLA_TRY((launch_row<SUM, TRAIN>(a, st)));
  return sum_grads(x, y, Wx, Wy, ws + w.dlogits, dWx, dbx, dWy, dby, dX, dY, ws + w.rowloss, losses, B, D, C, st);
}

extern "C" int mla_fusion_sum_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                                  float* out, float* out_a, float* out_v, int B, int D, int C, float bias_scale, void* stream) {
  const char* who = "mla_fusion_sum_fwd";
  FUSION_PTRS(who, x, y, Wx, bx, Wy, by, out, out_a, out_v);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  RowArgs a = row_args(B, D, C);
  a.x = x; a.y = y; a.Wa = Wx; a.ba = bx; a.Wb = Wy; a.bb = by;
  a.out = out; a.out_a = out_a; a.out_v = out_v; a.bias_scale = bias_scale;
  return launch_row<SUM, FWD>(a, (hipStream_t)stream);
}

extern "C" int mla_fusion_sum_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* dlogits, float* dWx,
                                  float* dbx, float* dWy, float* dby, float* dX, float* dY, float* ws, int B, int D, int C, float scale,
                                  void* stream) {
  const char* who = "mla_fusion_sum_bwd";
  FUSION_PTRS(who, x, y, Wx, Wy, dlogits, dWx, dbx, dWy, dby, dX, dY, ws);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  RowArgs a = row_args(B, D, C);
  a.dl_in = dlogits; a.dlogits = ws + w.dlogits; a.scale = scale;
  MLA_TRY((launch_row<SUM, BWD>(a, st)));
  return sum_grads(x, y, Wx, Wy, ws + w.dlogits, dWx, dbx, dWy, dby, dX, dY, nullptr, nullptr, B, D, C, st);
}

// ---- FiLM ---------------------------------------------------------------------------------------------------------------------------
static int film_hidden(const float* film, const float* W, const float* b, float* h, int B, int D, hipStream_t st) {
  HiddenJobs hj = {};
  hj.x[0] = film; hj.W[0] = W; hj.b[0] = b; hj.h[0] = h; hj.N[0] = 2 * D;
  return launch_hidden(hj, 1, B, D, st);
}

static int film_grads(const float* film, const float* W, const float* z, const float* dl, const float* dh, float* dW, float* db,
                      float* dWout, float* dbout, float* dfilm, const float* rowloss, float* loss, int B, int D, int C, hipStream_t st) {
  FusionJobs js;
  fusion_jobs_init(&js);
  MLA_TRY(fusion_jobs_add(&js, dl, z, nullptr, dWout, dbout, nullptr, B, C, D));
  MLA_TRY(fusion_jobs_add(&js, dh, film, W, dW, db, dfilm, B, 2 * D, D));
  return launch_grad(js, rowloss, loss, 1, B, st);
}

extern "C" int mla_fusion_film_ce_fwd_bwd(const float* film, const float* t, const float* W, const float* b, const float* Wout,
                                          const float* bout, const int64_t* labels, float* out, float* h, float* z, float* loss, float* dW,
                                          float* db, float* dWout, float* dbout, float* dfilm, float* dt, float* ws, int B, int D, int C,
                                          float inv_batch, void* stream) {
  const char* who = "mla_fusion_film_ce_fwd_bwd";
  FUSION_PTRS(who, film, t, W, b, Wout, bout, out, h, z, loss, dW, db, dWout, dbout, dfilm, dt, ws);
  MLA_TRY(fusion_check_labels(who, labels));
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  MLA_TRY(film_hidden(film, W, b, h, B, D, st));
  RowArgs a = row_args(B, D, C);
  a.y = t; a.Wa = Wout; a.ba = bout; a.h0 = h; a.z = z; a.labels = labels; a.out = out;
  a.dlogits = ws + w.dlogits; a.rowloss = ws + w.rowloss; a.dh = ws + w.dh; a.dt = dt; a.inv_batch = inv_batch;
  MLA_TRY((launch_row<FILM, TRAIN>(a, st)));
  return film_grads(film, W, z, ws + w.dlogits, ws + w.dh, dW, db, dWout, dbout, dfilm, ws + w.rowloss, loss, B, D, C, st);
}

extern "C" int mla_fusion_film_fwd(const float* film, const float* t, const float* W, const float* b, const float* Wout, const float* bout,
                                   float* out, float* h, float* z, int B, int D, int C, void* stream) {
  const char* who = "mla_fusion_film_fwd";
  FUSION_PTRS(who, film, t, W, b, Wout, bout, out, h, z);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  MLA_TRY(film_hidden(film, W, b, h, B, D, st));
  RowArgs a = row_args(B, D, C);
  a.y = t; a.Wa = Wout; a.ba = bout; a.h0 = h; a.z = z; a.out = out;
  return launch_row<FILM, FWD>(a, st);
}

extern "C" int mla_fusion_film_bwd(const float* film, const float* t, const float* W, const float* Wout, const float* h, const float* z,
                                   const float* dlogits, float* dW, float* db, float* dWout, float* dbout, float* dfilm, float* dt,
                                   float* ws, int B, int D, int C, float scale, void* stream) {
  const char* who = "mla_fusion_film_bwd";
  FUSION_PTRS(who, film, t, W, Wout, h, z, dlogits, dW, db, dWout, dbout, dfilm, dt, ws);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  RowArgs a = row_args(B, D, C);
  a.y = t; a.Wa = Wout; a.h0 = h; a.dl_in = dlogits; a.dlogits = ws + w.dlogits; a.dh = ws + w.dh; a.dt = dt; a.scale = scale;
  MLA_TRY((launch_row<FILM, BWD>(a, st)));
  return film_grads(film, W, z, ws + w.dlogits, ws + w.dh, dW, db, dWout, dbout, dfilm, nullptr, nullptr, B, D, C, st);
}

// ---- gated --------------------------------------------------------------------------------------------------------------------------
static int gated_hidden(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by, float* hx,
                        float* hy, int B, int D, hipStream_t st) {
  HiddenJobs hj = {};
  hj.x[0] = x; hj.W[0] = Wx; hj.b[0] = bx; hj.h[0] = hx; hj.N[0] = D;
  hj.x[1] = y; hj.W[1] = Wy; hj.b[1] = by; hj.h[1] = hy; hj.N[1] = D;
  return launch_hidden(hj, 2, B, D, st);
}

static int gated_grads(const float* x, const float* y, const float* Wx, const float* Wy, const float* z, const float* dl, const float* dh,
                       float* dWx, float* dbx, float* dWy, float* dby, float* dWout, float* dbout, float* dX, float* dY,
                       const float* rowloss, float* loss, int B, int D, int C, hipStream_t st) {
  FusionJobs js;
  fusion_jobs_init(&js);
  MLA_TRY(fusion_jobs_add(&js, dl, z, nullptr, dWout, dbout, nullptr, B, C, D));
  MLA_TRY(fusion_jobs_add(&js, dh, x, Wx, dWx, dbx, dX, B, D, D));
  MLA_TRY(fusion_jobs_add(&js, dh + (size_t)B * D, y, Wy, dWy, dby, dY, B, D, D));
  return launch_grad(js, rowloss, loss, 1, B, st);
}

extern "C" int mla_fusion_gated_ce_fwd_bwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy,
                                           const float* by, const float* Wout, const float* bout, const int64_t* labels, float* out,
                                           float* hx, float* hy, float* z, float* loss, float* dWx, float* dbx, float* dWy, float* dby,
                                           float* dWout, float* dbout, float* dX, float* dY, float* ws, int B, int D, int C, int x_gate,
                                           float inv_batch, void* stream) {
  const char* who = "mla_fusion_gated_ce_fwd_bwd";
  FUSION_PTRS(who, x, y, Wx, bx, Wy, by, Wout, bout, out, hx, hy, z, loss, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, ws);
  MLA_TRY(fusion_check_labels(who, labels));
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  MLA_TRY(gated_hidden(x, y, Wx, bx, Wy, by, hx, hy, B, D, st));
  RowArgs a = row_args(B, D, C);
  a.Wa = Wout; a.ba = bout; a.h0 = hx; a.h1 = hy; a.z = z; a.labels = labels; a.out = out; a.x_gate = x_gate != 0;
  a.dlogits = ws + w.dlogits; a.rowloss = ws + w.rowloss; a.dh = ws + w.dh; a.inv_batch = inv_batch;
  MLA_TRY((launch_row<GATED, TRAIN>(a, st)));
  return gated_grads(x, y, Wx, Wy, z, ws + w.dlogits, ws + w.dh, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, ws + w.rowloss, loss, B, D, C,
                     st);
}

extern "C" int mla_fusion_gated_fwd(const float* x, const float* y, const float* Wx, const float* bx, const float* Wy, const float* by,
                                    const float* Wout, const float* bout, float* out, float* hx, float* hy, float* z, int B, int D, int C,
                                    int x_gate, void* stream) {
  const char* who = "mla_fusion_gated_fwd";
  FUSION_PTRS(who, x, y, Wx, bx, Wy, by, Wout, bout, out, hx, hy, z);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  MLA_TRY(gated_hidden(x, y, Wx, bx, Wy, by, hx, hy, B, D, st));
  RowArgs a = row_args(B, D, C);
  a.Wa = Wout; a.ba = bout; a.h0 = hx; a.h1 = hy; a.z = z; a.out = out; a.x_gate = x_gate != 0;
  return launch_row<GATED, FWD>(a, st);
}

extern "C" int mla_fusion_gated_bwd(const float* x, const float* y, const float* Wx, const float* Wy, const float* Wout, const float* hx,
                                    const float* hy, const float* z, const float* dlogits, float* dWx, float* dbx, float* dWy, float* dby,
                                    float* dWout, float* dbout, float* dX, float* dY, float* ws, int B, int D, int C, int x_gate,
                                    float scale, void* stream) {
  const char* who = "mla_fusion_gated_bwd";
  FUSION_PTRS(who, x, y, Wx, Wy, Wout, hx, hy, z, dlogits, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, ws);
  MLA_TRY(fusion_check_shape(who, B, D, C));
  hipStream_t st = (hipStream_t)stream;
  const FusionWs w = fusion_ws_layout(B, D, C);
  RowArgs a = row_args(B, D, C);
  a.Wa = Wout; a.h0 = hx; a.h1 = hy; a.dl_in = dlogits; a.dlogits = ws + w.dlogits; a.dh = ws + w.dh; a.x_gate = x_gate != 0;
  a.scale = scale;
  MLA_TRY((launch_row<GATED, BWD>(a, st)));
  return gated_grads(x, y, Wx, Wy, z, ws + w.dlogits, ws + w.dh, dWx, dbx, dWy, dby, dWout, dbout, dX, dY, nullptr, nullptr, B, D, C, st);
}
