// AdversarialLoss (training/losses.py:150-289) around the implicit-GEMM convs: everything of a discriminator call that is not
// sfm_gemm16 / sfm_conv_wgrad16.  Activations are channels-last 16-bit rows [B, T, C]; every sum that crosses threads is taken
// in a fixed order (fp64 inside a workgroup, per-workgroup partials folded by one workgroup), so a step is bitwise repeatable.
//   sfm_adv_sn_fwd       spectral norm of all convs of one discriminator from a layer table: power iteration, sigma, W / sigma
//                        in sfm_gemm16's packed layout
//   sfm_adv_sn_bwd       tap-major dL/d(W / sigma) -> d weight_orig
//   sfm_adv_stage[_bwd]  [B, F, T] magnitudes or channels-last (re, im) -> zero-padded 16-bit rows, and the adjoint
//   sfm_adv_leaky[_bwd]  LeakyReLU(0.2) of the fp32 pre-activation (+ the L1 feature-matching sum), and dY of the gradient GEMMs
//   sfm_adv_pool[_bwd]   AvgPool1d(4, 2, 1), zero padding counted
//   sfm_adv_head[_bwd]   Conv1d(C, 1, 3, pad 1) as a dot product per row, fused with the MSE against a constant
#include "sfm_common.h"

namespace {

constexpr int NT = 256;                 // threads of every workgroup here (4 waves)
constexpr int SN_COLS = 16;             // int64 words per layer of the spectral-norm table
constexpr float SLOPE = 0.2f;

// sum of v over the workgroup, the same value in every thread; fixed order: butterfly per wave, then waves 0..3
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();                      // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float leaky(float z) { return z > 0.f ? z : SLOPE * z; }

// The backward of one objective carries a power of two S on everything it rounds to 16 bits (the dY of the gradient GEMMs, and so
// their fp32 results), taken out again, exactly, where a gradient leaves in fp32: S = 2^k with |g * cnorm| * S in [32, 64), g =
// the objective's incoming gradient, cnorm = its largest static coefficient (2 / (3 B T') of the heads, 1 / (3 numel) of the
// feature terms).  At B 256 x 250 frames that coefficient is ~1e-5 and dY a few 1e-7 behind it: under fp16's normal range for any
// g near 1, whatever the caller's loss scale does.  A pure function of (g, cnorm): every kernel of the pass computes the same S.
__device__ __forceinline__ float adv_scale(const float* g, float cnorm) {
  if (!g) return 1.f;
  const float a = fabsf(g[0] * cnorm);
  if (!(a > 0.f) || !(a < 3.0e38f)) return 1.f;
  int e;
  (void)frexpf(a, &e);                  // a = m 2^e, m in [0.5, 1)
  e = 6 - e;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  return ldexpf(1.f, e);
}

// The forward keeps every GEMM operand as a pair of 16-bit words, v = hi + lo / LO_SCALE (hi = v rounded, lo = the rounding error
// scaled back into the format's normal range), and runs hi x hi + (lo x hi + hi x lo) / LO_SCALE: the pre-activations then carry
// ~2^-20 instead of 2^-11 (fp16) / 2^-8 (bf16).  LeakyReLU and the L1 of the feature term have kinks; with single 16-bit operands
// a few pre-activations per tensor land on the other side of zero and each costs 0.8 |dz| (2 w) of the gradient: 1e-2..1e-1 of
// its norm on small tensors, however exact the backward is.  The backward stays on the hi words alone (it is smooth).
constexpr float LO_SCALE = SFM_ADV_LO_SCALE;  // (the header's literal, as a float: the products below are fp32)
template <class T>
__device__ __forceinline__ void split16(float v, u16& hi, u16& lo) {
  hi = T::from_f32(v);
  lo = T::from_f32((v - T::to_f32(hi)) * LO_SCALE);
}

template <class T>
__device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = T::to_f32((u16)(v[i] & 0xffffu));
    f[2 * i + 1] = T::to_f32((u16)(v[i] >> 16));
  }
}

// ---- spectral norm ---------------------------------------------------------------------------------------------------------
// table row: {weight_orig [N][Cin][k], bias [N], weight_u [N], weight_v [Cin k], N, Cin, k, Cp, Npad, Kpad, off16, off32}
// packed (hi) and packed_lo + off16: W / sigma as [Npad][Kpad] 16-bit pairs (split16), column tap * Cp + ci, zero elsewhere
// saved + off32:  bias [Npad] | u [N] | v [Cin k] | W v [N] | sigma [1]   (this call's vectors: its backward needs them)
template <class T>
__global__ __launch_bounds__(NT) void adv_sn_fwd_kernel(const long long* __restrict__ table, u16* __restrict__ packed,
                                                        u16* __restrict__ packed_lo, float* __restrict__ saved, int training,
                                                        float eps) {
  __shared__ double red[4];
  const long long* e = table + (long long)blockIdx.x * SN_COLS;
  const float* W = (const float*)e[0];
  const float* bias = (const float*)e[1];
  float* ubuf = (float*)e[2];
  float* vbuf = (float*)e[3];
  const int N = (int)e[4], Cin = (int)e[5], ks = (int)e[6], Cp = (int)e[7], Npad = (int)e[8], Kpad = (int)e[9];
  const int K = Cin * ks;
  u16* P = packed + e[10];
  u16* Plo = packed_lo + e[10];
  float* bp = saved + e[11];
  float* us = bp + Npad;
  float* vs = us + N;
  float* ss = vs + K;
  float* sig = ss + N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if (training) {                                       // v <- normalize(W^T u)
    double sq = 0.0;
    for (int j = tid; j < K; j += NT) {
      double a = 0.0;
      for (int i = 0; i < N; ++i) a += (double)W[(long long)i * K + j] * (double)ubuf[i];
      vs[j] = (float)a;
      sq += (double)(float)a * (double)(float)a;
    }
    const float nrm = fmaxf((float)sqrt(block_sum(sq, red)), eps);
    for (int j = tid; j < K; j += NT) vs[j] = vs[j] / nrm;
  } else {
    for (int j = tid; j < K; j += NT) vs[j] = vbuf[j];
    for (int i = tid; i < N; i += NT) us[i] = ubuf[i];
  }
  __syncthreads();
  for (int i = wave; i < N; i += NT / 64) {             // W v, one wave per row
    double a = 0.0;
    for (int j = lane; j < K; j += 64) a += (double)W[(long long)i * K + j] * (double)vs[j];
    a = wave_sum_d(a);
    if (lane == 0) ss[i] = (float)a;
  }
  __syncthreads();
  if (training) {                                       // u <- normalize(W v)
    double sq = 0.0;
    for (int i = tid; i < N; i += NT) sq += (double)ss[i] * (double)ss[i];
    const float nrm = fmaxf((float)sqrt(block_sum(sq, red)), eps);
    for (int i = tid; i < N; i += NT) us[i] = ss[i] / nrm;
    __syncthreads();
  }
  double d = 0.0;
  for (int i = tid; i < N; i += NT) d += (double)us[i] * (double)ss[i];
  const float sigma = (float)block_sum(d, red);         // u^T W v
  if (tid == 0) sig[0] = sigma;
  if (training) {
    for (int j = tid; j < K; j += NT) vbuf[j] = vs[j];
    for (int i = tid; i < N; i += NT) ubuf[i] = us[i];
  }
  for (int n = tid; n < Npad; n += NT) bp[n] = n < N ? bias[n] : 0.f;
  const int total = Npad * Kpad;
  for (int idx = tid; idx < total; idx += NT) {
    const int n = idx / Kpad, kk = idx - n * Kpad;
    const int tap = kk / Cp, ci = kk - tap * Cp;
    float v = 0.f;
    if (n < N && tap < ks && ci < Cin) v = W[(long long)n * K + ci * ks + tap] / sigma;
    split16<T>(v, P[idx], Plo[idx]);
  }
}

// d weight_orig = (G - <G, W / sigma> u v^T) / sigma / S;  G [N][k][Cp] tap-major (conv_wgrad16), W and dW [N][Cin][k];
// d bias = db_in / S (G and db_in carry the pass's scale S, see adv_scale)
__global__ __launch_bounds__(NT) void adv_sn_bwd_kernel(const float* __restrict__ G, const float* __restrict__ W,
                                                        const float* __restrict__ u, const float* __restrict__ v,
                                                        const float* __restrict__ sig, float* __restrict__ dW,
                                                        const float* __restrict__ db_in, float* __restrict__ db, const float* g,
                                                        float cnorm, int N, int Cin, int ks, int Cp, int accumulate) {
  __shared__ double red[4];
  const int K = Cin * ks, total = N * K;
  double a = 0.0;
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int n = idx / K, r = idx - n * K, ci = r / ks, tap = r - ci * ks;
    a += (double)G[((long long)n * ks + tap) * Cp + ci] * (double)W[idx];
  }
  const float sigma = sig[0], unscale = 1.f / adv_scale(g, cnorm);
  const float inner = (float)(block_sum(a, red) / (double)sigma);
  for (int idx = threadIdx.x; idx < total; idx += NT) {
    const int n = idx / K, r = idx - n * K, ci = r / ks, tap = r - ci * ks;
    const float d = (G[((long long)n * ks + tap) * Cp + ci] - inner * u[n] * v[r]) / sigma * unscale;
    dW[idx] = accumulate ? dW[idx] + d : d;
  }
  if (db_in)
    for (int n = threadIdx.x; n < N; n += NT) db[n] = accumulate ? db[n] + db_in[n] * unscale : db_in[n] * unscale;
}

// ---- ordered folds ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void adv_fold_scalar_kernel(const double* __restrict__ ws, int n, double* __restrict__ loss,
                                                             float scale, int accumulate) {
  __shared__ double red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += NT) a += ws[i];
  a = block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = (accumulate ? loss[0] : 0.0) + (double)scale * a;
}

__global__ __launch_bounds__(NT) void adv_fold_cols_kernel(const float* __restrict__ ws, int S, int cols, float* __restrict__ out) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= cols) return;
  double a = 0.0;
  for (int s = 0; s < S; ++s) a += (double)ws[(long long)s * cols + j];
  out[j] = (float)a;
}

// ---- input staging ---------------------------------------------------------------------------------------------------------
// x [B][F][T] fp32 -> x16 [B][T][Cp] (columns >= F zero) and, when asked for, x32 [B][T][F]: a 32 x 32 tile through LDS
template <class T>
__global__ __launch_bounds__(NT) void adv_stage_bft_kernel(const float* __restrict__ x, u16* __restrict__ x16, u16* __restrict__ x16lo,
                                                           float* __restrict__ x32, int F, int Tn, int Cp) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + ty + 8 * r, t = t0 + tx;
    tile[ty + 8 * r][tx] = (c < F && t < Tn) ? x[((long long)b * F + c) * Tn + t] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = t0 + ty + 8 * r, c = c0 + tx;
    if (t < Tn && c < Cp) {
      const float v = tile[tx][ty + 8 * r];
      split16<T>(v, x16[((long long)b * Tn + t) * Cp + c], x16lo[((long long)b * Tn + t) * Cp + c]);
      if (x32 && c < F) x32[((long long)b * Tn + t) * F + c] = v;
    }
  }
}

// the adjoint: d [B][T][Cp] fp32 -> dx [B][F][T], every element written
__global__ __launch_bounds__(NT) void adv_stage_bft_bwd_kernel(const float* __restrict__ d, float* __restrict__ dx, const float* g,
                                                               float cnorm, int F, int Tn, int Cp) {
  __shared__ float tile[32][33];
  const float unscale = 1.f / adv_scale(g, cnorm);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, b = blockIdx.z;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = t0 + ty + 8 * r, c = c0 + tx;
    tile[ty + 8 * r][tx] = (t < Tn && c < F) ? d[((long long)b * Tn + t) * Cp + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = c0 + ty + 8 * r, t = t0 + tx;
    if (c < F && t < Tn) dx[((long long)b * F + c) * Tn + t] = tile[tx][ty + 8 * r] * unscale;
  }
}

// (re, im) [rows][F] -> sqrt(re^2 + im^2 + 1e-8) as x16 [rows][Cp] and x32 [rows][F]
template <class T>
__global__ __launch_bounds__(NT) void adv_stage_pair_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                            u16* __restrict__ x16, u16* __restrict__ x16lo,
                                                            float* __restrict__ x32, long long rows, int F,
                                                            int Cp) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= rows * Cp) return;
  const long long row = idx / Cp;
  const int c = (int)(idx - row * Cp);
  float v = 0.f;
  if (c < F) {
    const float a = re[row * F + c], b = im[row * F + c];
    v = sqrtf(a * a + b * b + 1e-8f);
    if (x32) x32[row * F + c] = v;
  }
  split16<T>(v, x16[idx], x16lo[idx]);
}

__global__ __launch_bounds__(NT) void adv_stage_pair_bwd_kernel(const float* __restrict__ d, const float* __restrict__ re,
                                                                const float* __restrict__ im, float* __restrict__ dre,
                                                                float* __restrict__ dim, const float* g, float cnorm,
                                                                long long rows, int F, int Cp) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= rows * F) return;
  const long long row = idx / F;
  const int c = (int)(idx - row * F);
  const float a = re[idx], b = im[idx];
  const float dm = d[row * Cp + c] / adv_scale(g, cnorm) / sqrtf(a * a + b * b + 1e-8f);
  dre[idx] = dm * a;
  dim[idx] = dm * b;
}

// ---- LeakyReLU -------------------------------------------------------------------------------------------------------------
// a16 = leaky(z); with zr (the real pass's pre-activation) also ws[block] = sum |leaky(z) - leaky(zr)| over the block's elements
template <class T>
__global__ __launch_bounds__(NT) void adv_leaky_kernel(const float* __restrict__ z, const float* __restrict__ zr,
                                                       u16* __restrict__ a16, u16* __restrict__ a16lo,
                                                       double* __restrict__ ws, long long n) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long i = ((long long)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * NT * 4) {
    const f32x4 v = *(const f32x4*)(z + i);
    float a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = leaky(v[j]);
    if (zr) {
      const f32x4 r = *(const f32x4*)(zr + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += (double)fabsf(a[j] - leaky(r[j]));
    }
    u16 h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split16<T>(a[j], h[j], l[j]);
    u32x2 o = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
    u32x2 ol = {(uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16)};
    *(u32x2*)(a16 + i) = o;
    *(u32x2*)(a16lo + i) = ol;
  }
  if (zr) {
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc;
  }
}

// dz16 = (inc + S * wfm * g * sign(leaky(z) - leaky(zr))) * (z > 0 ? 1 : 0.2); inc carries S already
template <class T>
__global__ __launch_bounds__(NT) void adv_leaky_bwd_kernel(const float* __restrict__ inc, const float* __restrict__ z,
                                                           const float* __restrict__ zr, const float* __restrict__ g, float wfm,
                                                           float cnorm, u16* __restrict__ dz16, long long n) {
  const float w = zr ? wfm * g[0] * adv_scale(g, cnorm) : 0.f;
  for (long long i = ((long long)blockIdx.x * NT + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * NT * 4) {
    const f32x4 v = *(const f32x4*)(z + i);
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (inc) d = *(const f32x4*)(inc + i);
    if (zr) {
      const f32x4 r = *(const f32x4*)(zr + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float df = leaky(v[j]) - leaky(r[j]);
        d[j] += df > 0.f ? w : (df < 0.f ? -w : 0.f);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= v[j] > 0.f ? 1.f : SLOPE;
    u32x2 o = {T::pack(d[0], d[1]), T::pack(d[2], d[3])};
    *(u32x2*)(dz16 + i) = o;
  }
}

// ---- AvgPool1d(4, 2, 1) on channels-last rows --------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(NT) void adv_pool_kernel(const float* __restrict__ in, float* __restrict__ out32,
                                                      u16* __restrict__ out16, u16* __restrict__ out16lo, int B, int Tin,
                                                      int Tout, int F, int Cp) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long long)B * Tout * Cp) return;
  const long long row = idx / Cp;
  const int c = (int)(idx - row * Cp), b = (int)(row / Tout), o = (int)(row - (long long)b * Tout);
  float v = 0.f;
  if (c < F) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = 2 * o - 1 + j;
      if (t >= 0 && t < Tin) v += in[((long long)b * Tin + t) * F + c];
    }
    v *= 0.25f;
    if (out32) out32[row * F + c] = v;
  }
  split16<T>(v, out16[idx], out16lo[idx]);
}

// dx [B][Tin][Cp] += 0.25 * sum of dnext [B][Tout][Cp] over the windows that hold t (a gather: no atomics)
__global__ __launch_bounds__(NT) void adv_pool_bwd_kernel(const float* __restrict__ dnext, float* __restrict__ dx, int B, int Tin,
                                                          int Tout, int Cp) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long long)B * Tin * Cp) return;
  const long long row = idx / Cp;
  const int c = (int)(idx - row * Cp), b = (int)(row / Tin), t = (int)(row - (long long)b * Tin);
  float v = 0.f;
  for (int o = (t - 1) >> 1; o <= (t + 1) >> 1; ++o)     // 2 o - 1 <= t <= 2 o + 2
    if (o >= 0 && o < Tout && 2 * o - 1 <= t && t <= 2 * o + 2) v += dnext[((long long)b * Tout + o) * Cp + c];
  dx[idx] += 0.25f * v;
}

// ---- head: Conv1d(C, 1, 3, pad 1) + MSE against a constant --------------------------------------------------------------------
// one wave per row (b, t); w16 [3][C] tap-major; ws[block] = sum over the block's rows of (out - target)^2
template <class T>
__global__ __launch_bounds__(NT) void adv_head_kernel(const u16* __restrict__ a16, const u16* __restrict__ a16lo,
                                                      const u16* __restrict__ w16, const u16* __restrict__ w16lo,
                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                      double* __restrict__ ws, float target, int B, int Tn, int C) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wave, rows = (long long)B * Tn;
  double sq = 0.0;
  if (row < rows) {
    const int b = (int)(row / Tn), t = (int)(row - (long long)b * Tn), C8 = C >> 3;
    float acc = 0.f;
    for (int q = lane; q < 3 * C8; q += 64) {
      const int tap = q / C8, c = (q - tap * C8) * 8, tt = t - 1 + tap;
      if (tt < 0 || tt >= Tn) continue;
      float x[8], w[8];
      unpack8<T>(*(const u32x4*)(a16 + ((long long)b * Tn + tt) * C + c), x);
      unpack8<T>(*(const u32x4*)(w16 + tap * C + c), w);
      float xl[8], wl[8];
      unpack8<T>(*(const u32x4*)(a16lo + ((long long)b * Tn + tt) * C + c), xl);
      unpack8<T>(*(const u32x4*)(w16lo + tap * C + c), wl);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc = fmaf(fmaf(xl[j], 1.f / LO_SCALE, x[j]), fmaf(wl[j], 1.f / LO_SCALE, w[j]), acc);
    }
    acc = wave_sum(acc) + bias[0];
    if (lane == 0) {
      out[row] = acc;
      sq = (double)(acc - target) * (double)(acc - target);
    }
  }
  sq = block_sum(sq, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = sq;
}

// da [B][T][C] fp32 = S * sum_tap dout[b, t + 1 - tap] w[tap][c],  dout = g * coef * (out - target)
template <class T>
__global__ __launch_bounds__(NT) void adv_head_da_kernel(const u16* __restrict__ w16, const float* __restrict__ out,
                                                         const float* __restrict__ g, float coef, float cnorm, float target,
                                                         float* __restrict__ da, int B, int Tn, int C) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= (long long)B * Tn * C) return;
  const long long row = idx / C;
  const int c = (int)(idx - row * C), b = (int)(row / Tn), t = (int)(row - (long long)b * Tn);
  const float s = g[0] * coef * adv_scale(g, cnorm);
  float v = 0.f;
#pragma unroll
  for (int tap = 0; tap < 3; ++tap) {
    const int to = t + 1 - tap;
    if (to >= 0 && to < Tn) v = fmaf(s * (out[(long long)b * Tn + to] - target), T::to_f32(w16[tap * C + c]), v);
  }
  da[idx] = v;
}

// ws[chunk][3 C + 1]: the chunk's rows' share of dw [3][C] (tap-major) and db
constexpr int HEAD_ROWS = 64;
template <class T>
__global__ __launch_bounds__(NT) void adv_head_dw_kernel(const u16* __restrict__ a16, const float* __restrict__ out,
                                                         const float* __restrict__ g, float coef, float target,
                                                         float* __restrict__ ws, int B, int Tn, int C) {
  const long long rows = (long long)B * Tn, r0 = (long long)blockIdx.x * HEAD_ROWS;
  const long long r1 = r0 + HEAD_ROWS < rows ? r0 + HEAD_ROWS : rows;
  const int cols = 3 * C + 1;
  const float s = g[0] * coef;
  for (int j = threadIdx.x; j < cols; j += NT) {
    float acc = 0.f;
    if (j == 3 * C) {
      for (long long r = r0; r < r1; ++r) acc += s * (out[r] - target);
    } else {
      const int tap = j / C, c = j - tap * C;
      for (long long r = r0; r < r1; ++r) {
        const int b = (int)(r / Tn), t = (int)(r - (long long)b * Tn), tt = t - 1 + tap;
        if (tt >= 0 && tt < Tn) acc = fmaf(s * (out[r] - target), T::to_f32(a16[((long long)b * Tn + tt) * C + c]), acc);
      }
    }
    ws[(long long)blockIdx.x * cols + j] = acc;
  }
}

constexpr int EW_MAX_BLOCKS = 2048;
inline int ew_grid(long long n4) {
  const long long g = sfm_capped_blocks(n4, NT, EW_MAX_BLOCKS);
  return (int)(g < 1 ? 1 : g);
}
constexpr int HEAD_WAVES = NT / 64;        // adv_head_kernel: one row per wave, one partial per workgroup
inline long long head_blocks(int B, int T) { return ((long long)B * T + HEAD_WAVES - 1) / HEAD_WAVES; }
inline long long head_chunks(int B, int T) { return ((long long)B * T + HEAD_ROWS - 1) / HEAD_ROWS; }

}  // namespace

#define ADV_DT(dtype, STMT)                          \
  if (dtype == SFM_DT_BF16) { typedef BF16 DT; STMT } \
  else if (dtype == SFM_DT_F16) { typedef F16 DT; STMT } \
  else return SFM_ERR_ARG;

extern "C" {

int sfm_adv_sn_fwd(const long long* table, int n_layers, void* packed, void* packed_lo, float* saved, int training, float eps,
                   int dtype, void* stream) {
  if (!table || !packed || !packed_lo || !saved) return SFM_ERR_ARG;
  if (n_layers <= 0 || n_layers > 64) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  ADV_DT(dtype, SFM_LAUNCH(adv_sn_fwd_kernel<DT>, dim3(n_layers), dim3(NT), 0, st, table, (u16*)packed, (u16*)packed_lo, saved,
                           training, eps);)
  return SFM_OK;
}

int sfm_adv_sn_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma, float* dW,
                   const float* db_in, float* db, const float* g, float cnorm, int N, int Cin, int ksize, int Cp, int accumulate,
                   void* stream) {
  if (!G || !W || !u || !v || !sigma || !dW || (db_in && !db)) return SFM_ERR_ARG;
  if (N <= 0 || Cin <= 0 || ksize <= 0 || Cp < Cin || (long long)N * Cin * ksize >= (1LL << 31)) return SFM_ERR_SHAPE;
  SFM_LAUNCH(adv_sn_bwd_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, G, W, u, v, sigma, dW, db_in, db, g, cnorm, N, Cin,
             ksize, Cp, accumulate);
  return SFM_OK;
}

int sfm_adv_stage(const float* x, const float* im, void* x16, void* x16lo, float* x32, int B, int F, int T, int Cp, int pair,
                  int dtype, void* stream) {
  if (!x || !x16 || !x16lo || (pair && !im)) return SFM_ERR_ARG;
  if (B <= 0 || F <= 0 || T <= 0 || Cp < F || (Cp % 8) != 0 || B > 65535) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (pair) {
    const long long n = (long long)B * T * Cp;
    if ((n + NT - 1) / NT >= (1LL << 31)) return SFM_ERR_SHAPE;
    ADV_DT(dtype, SFM_LAUNCH(adv_stage_pair_kernel<DT>, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, x, im, (u16*)x16, (u16*)x16lo,
                             x32, (long long)B * T, F, Cp);)
  } else {
    if ((Cp + 31) / 32 > 65535) return SFM_ERR_SHAPE;
    ADV_DT(dtype, SFM_LAUNCH(adv_stage_bft_kernel<DT>, dim3((T + 31) / 32, (Cp + 31) / 32, B), dim3(NT), 0, st, x, (u16*)x16, (u16*)x16lo, x32,
                             F, T, Cp);)
  }
  return SFM_OK;
}

int sfm_adv_stage_bwd(const float* d, const float* re, const float* im, float* dx, float* dx_im, const float* g, float cnorm, int B,
                      int F, int T, int Cp, int pair, void* stream) {
  if (!d || !dx || (pair && (!re || !im || !dx_im))) return SFM_ERR_ARG;
  if (B <= 0 || F <= 0 || T <= 0 || Cp < F || B > 65535) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (pair) {
    const long long n = (long long)B * T * F;
    if ((n + NT - 1) / NT >= (1LL << 31)) return SFM_ERR_SHAPE;
    SFM_LAUNCH(adv_stage_pair_bwd_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, d, re, im, dx, dx_im,
               g, cnorm, (long long)B * T, F, Cp);
  } else {
    if ((F + 31) / 32 > 65535) return SFM_ERR_SHAPE;
    SFM_LAUNCH(adv_stage_bft_bwd_kernel, dim3((T + 31) / 32, (F + 31) / 32, B), dim3(NT), 0, st, d, dx, g, cnorm, F, T, Cp);
  }
  return SFM_OK;
}

// sized for ew_grid's cap, whatever n: one partial per workgroup
long long sfm_adv_leaky_ws_doubles(long long n) { (void)n; return EW_MAX_BLOCKS; }
int sfm_adv_leaky(const float* z, const float* z_real, void* a16, void* a16lo, double* ws, double* loss, float scale, long long n,
                  int dtype, void* stream) {
  if (!z || !a16 || !a16lo || (z_real && (!ws || !loss))) return SFM_ERR_ARG;
  if (n <= 0 || (n % 4) != 0) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int grid = ew_grid(n / 4);
  ADV_DT(dtype, SFM_LAUNCH(adv_leaky_kernel<DT>, dim3(grid), dim3(NT), 0, st, z, z_real, (u16*)a16, (u16*)a16lo, ws, n);)
  if (z_real) SFM_LAUNCH(adv_fold_scalar_kernel, dim3(1), dim3(NT), 0, st, (const double*)ws, grid, loss, scale, 1);
  return SFM_OK;
}

int sfm_adv_leaky_bwd(const float* incoming, const float* z, const float* z_real, const float* g, float w_fm, float cnorm,
                      void* dz16, long long n, int dtype, void* stream) {
  if (!z || !dz16 || (z_real && !g) || (!incoming && !z_real)) return SFM_ERR_ARG;
  if (n <= 0 || (n % 4) != 0) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  ADV_DT(dtype, SFM_LAUNCH(adv_leaky_bwd_kernel<DT>, dim3(ew_grid(n / 4)), dim3(NT), 0, st, incoming, z, z_real, g, w_fm,
                           cnorm, (u16*)dz16, n);)
  return SFM_OK;
}

int sfm_adv_pool(const float* in32, float* out32, void* out16, void* out16lo, int B, int Tin, int F, int Cp, int dtype,
                 void* stream) {
  if (!in32 || !out16 || !out16lo) return SFM_ERR_ARG;
  const int Tout = Tin / 2;                              // (Tin + 2 - 4) / 2 + 1
  if (B <= 0 || Tin < 2 || F <= 0 || Cp < F) return SFM_ERR_SHAPE;
  const long long n = (long long)B * Tout * Cp;
  if ((n + NT - 1) / NT >= (1LL << 31)) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  ADV_DT(dtype, SFM_LAUNCH(adv_pool_kernel<DT>, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, in32, out32, (u16*)out16,
                           (u16*)out16lo, B,
                           Tin, Tout, F, Cp);)
  return SFM_OK;
}

int sfm_adv_pool_bwd(const float* dnext, float* dx, int B, int Tin, int Cp, void* stream) {
  if (!dnext || !dx) return SFM_ERR_ARG;
  if (B <= 0 || Tin < 2 || Cp <= 0) return SFM_ERR_SHAPE;
  const long long n = (long long)B * Tin * Cp;
  if ((n + NT - 1) / NT >= (1LL << 31)) return SFM_ERR_SHAPE;
  SFM_LAUNCH(adv_pool_bwd_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, dnext, dx, B, Tin,
             Tin / 2, Cp);
  return SFM_OK;
}

long long sfm_adv_head_ws_doubles(int B, int T) { return B > 0 && T > 0 ? head_blocks(B, T) : 0; }
int sfm_adv_head(const void* a16, const void* a16lo, const void* w16, const void* w16lo, const float* bias, float* out, double* ws,
                 double* loss, float target,
                 float scale, int B, int T, int C, int dtype, void* stream) {
  if (!a16 || !a16lo || !w16 || !w16lo || !bias || !out || !ws || !loss) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || C <= 0 || (C % 8) != 0) return SFM_ERR_SHAPE;
  const long long blocks = head_blocks(B, T);
  if (blocks >= (1LL << 31)) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  ADV_DT(dtype, SFM_LAUNCH(adv_head_kernel<DT>, dim3((unsigned)blocks), dim3(NT), 0, st, (const u16*)a16, (const u16*)a16lo,
                           (const u16*)w16, (const u16*)w16lo, bias, out,
                           ws, target, B, T, C);)
  SFM_LAUNCH(adv_fold_scalar_kernel, dim3(1), dim3(NT), 0, st, (const double*)ws, (int)blocks, loss, scale, 1);
  return SFM_OK;
}

// ws[chunk][3 C + 1] of adv_head_dw_kernel
long long sfm_adv_head_bwd_ws_floats(int B, int T, int C) { return B > 0 && T > 0 && C > 0 ? head_chunks(B, T) * (3 * C + 1) : 0; }
int sfm_adv_head_bwd(const void* a16, const void* w16, const float* out, const float* g, float coef, float cnorm, float target,
                     float* da, float* dwb, float* ws, int B, int T, int C, int dtype, void* stream) {
  if (!a16 || !w16 || !out || !g || !da || (dwb && !ws)) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || C <= 0) return SFM_ERR_SHAPE;
  const long long n = (long long)B * T * C, chunks = head_chunks(B, T);
  if ((n + NT - 1) / NT >= (1LL << 31)) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  ADV_DT(dtype, SFM_LAUNCH(adv_head_da_kernel<DT>, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, st, (const u16*)w16, out, g,
                           coef, cnorm, target, da, B, T, C);)
  if (dwb) {
    ADV_DT(dtype, SFM_LAUNCH(adv_head_dw_kernel<DT>, dim3((unsigned)chunks), dim3(NT), 0, st, (const u16*)a16, out, g, coef, target,
                             ws, B, T, C);)
    SFM_LAUNCH(adv_fold_cols_kernel, dim3((3 * C + 1 + NT - 1) / NT), dim3(NT), 0, st, (const float*)ws, (int)chunks, 3 * C + 1,
               dwb);
  }
  return SFM_OK;
}

}  // extern "C"
