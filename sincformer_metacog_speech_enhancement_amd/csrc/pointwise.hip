// HBM-bound kernels of the path: normalisations, depthwise conv, layout packs,
// mask epilogue, overlap-add, sinc filter synthesis.  All are coalesced
// streaming kernels (wave = 64 lanes, shuffles for row statistics, LDS halos).
#include "sfm_common.h"

// ---------------------------------------------------------------------------
// LayerNorm over the last dim (nn.LayerNorm; models/conformer.py:43,68,107,150,
// agents/msa.py:44,47).  One wave per row, two-pass statistics in registers.
// Writes a 16-bit copy (GEMM operand) and/or an fp32 copy; optional erf-GELU.
// ---------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bsh, u16* out16, float* out32,
                                                        int M, int D, int ldx, int ld16, int ld32, float eps, int act) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (long long)row * ldx;
  float v[8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int d = lane + 64 * i;
    v[i] = (d < D) ? xr[d] : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int d = lane + 64 * i;
    float c = (d < D) ? (v[i] - mean) : 0.f;
    q += c * c;
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int d = lane + 64 * i;
    if (d < D) {
      float y = (v[i] - mean) * rstd * w[d] + bsh[d];
      if (act == 1) y = gelu_erf(y);
      if (out16) out16[(long long)row * ld16 + d] = T::from_f32(y);
      if (out32) out32[(long long)row * ld32 + d] = y;
    }
  }
}

// D = 256 (every LayerNorm of the Conformer blocks): a wave takes TWO rows per trip, a lane 4 consecutive columns of each
// (16-byte loads, 8- or 16-byte stores), row sums by DPP adds.  The general kernel above moves 4 bytes per lane per instruction.
template <class T>
__global__ __launch_bounds__(256) void layernorm256_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bsh, u16* out16, float* out32, int M,
                                                           int ldx, int ld16, int ld32, float eps, int act) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;
  if (row0 >= M) return;
  const bool two = row0 + 1 < M;
  const f32x4 gw = *reinterpret_cast<const f32x4*>(w + 4 * lane), gb = *reinterpret_cast<const f32x4*>(bsh + 4 * lane);
  f32x4 v[2];
  v[0] = *reinterpret_cast<const f32x4*>(x + (long long)row0 * ldx + 4 * lane);
  v[1] = *reinterpret_cast<const f32x4*>(x + (long long)(two ? row0 + 1 : row0) * ldx + 4 * lane);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r == 1 && !two) break;
    const float mean = wave_sum_dpp((v[r][0] + v[r][1]) + (v[r][2] + v[r][3])) * (1.0f / 256.0f);
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = v[r][j] - mean;
    const float rstd = rsqrtf(wave_sum_dpp((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / 256.0f) + eps);
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      y[j] = d[j] * rstd * gw[j] + gb[j];
      if (act == 1) y[j] = gelu_erf(y[j]);
    }
    const long long row = row0 + r;
    if (out16) {
      u32x2 pk;
      pk[0] = pack2<T>(y[0], y[1]);
      pk[1] = pack2<T>(y[2], y[3]);
      *reinterpret_cast<u32x2*>(out16 + row * ld16 + 4 * lane) = pk;
    }
    if (out32) *reinterpret_cast<f32x4*>(out32 + row * ld32 + 4 * lane) = f32x4{y[0], y[1], y[2], y[3]};
  }
}

extern "C" int sfm_layernorm(const float* x, const float* w, const float* b, void* out16, float* out32, int M, int D,
                             int ldx, int ld16, int ld32, float eps, int act, int dtype, void* stream) {
  if (!x || !w || !b || (!out16 && !out32)) return SFM_ERR_ARG;
  if (M <= 0 || D <= 0 || D > SFM_LAYERNORM_MAX_D) return SFM_ERR_SHAPE;
  // every row stride must cover the D normalised columns, or rows would overlap (and the last one run past its buffer)
  if (ldx < D || (out16 && ld16 < D) || (out32 && ld32 < D)) return SFM_ERR_SHAPE;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  const bool vec = D == 256 && (ldx % 4 == 0) && (((uintptr_t)x | (uintptr_t)w | (uintptr_t)b) % 16 == 0) &&
                   (!out16 || ((ld16 % 4 == 0) && ((uintptr_t)out16 % 8 == 0))) &&
                   (!out32 || ((ld32 % 4 == 0) && ((uintptr_t)out32 % 16 == 0)));
  if (vec) {
    dim3 grid2((M + 7) / 8), block2(256);
    if (dtype == SFM_DT_F16)
      SFM_LAUNCH((layernorm256_kernel<F16>), grid2, block2, 0, (hipStream_t)stream, x, w, b, (u16*)out16, out32, M, ldx, ld16, ld32,
                 eps, act);
    else
      SFM_LAUNCH((layernorm256_kernel<BF16>), grid2, block2, 0, (hipStream_t)stream, x, w, b, (u16*)out16, out32, M, ldx, ld16, ld32,
                 eps, act);
    return SFM_OK;
  }
  dim3 grid((M + 3) / 4), block(256);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((layernorm_kernel<F16>), grid, block, 0, (hipStream_t)stream, x, w, b, (u16*)out16, out32, M, D,
                       ldx, ld16, ld32, eps, act);
  else
    SFM_LAUNCH((layernorm_kernel<BF16>), grid, block, 0, (hipStream_t)stream, x, w, b, (u16*)out16, out32, M,
                       D, ldx, ld16, ld32, eps, act);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// GroupNorm (agents/perception.py:157,169,176,180,196,199,204).  Statistics
// arrive as per-tile partial (sum, sumsq) written by the producing GEMM's
// epilogue; gn_finalize reduces them (fp64) into per-(batch, channel)
// scale/shift; gn_apply normalises (+ optional second branch, + GELU).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gn_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ w,
                                                         const float* __restrict__ bsh, float* scale, float* shift,
                                                         int P, int G, int C, double count, float eps) {
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  double s = 0.0, q = 0.0;
  // eight partial slots per lane per trip, loaded together (a rolled one-slot loop pays a memory round trip per slot: 8 in a
  // row at P = 500, which was this kernel's whole 8 us); same summation order
  for (int i0 = lane; i0 < P; i0 += 64 * 8) {
    f32x2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + 64 * k < P ? i0 + 64 * k : P - 1;
      v[k] = *reinterpret_cast<const f32x2*>(partial + (((long long)b * P + i) * G + g) * 2);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i0 + 64 * k < P) {
        s += (double)v[k][0];
        q += (double)v[k][1];
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  const double mean = s / count;
  double var = q / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const int cpg = C / G;
  for (int i = lane; i < cpg; i += 64) {
    int c = g * cpg + i;
    float sc = w[c] * rstd;
    scale[(long long)b * C + c] = sc;
    shift[(long long)b * C + c] = bsh[c] - (float)mean * sc;
  }
}

extern "C" int sfm_gn_finalize(const float* partial, const float* w, const float* b, float* scale, float* shift, int B,
                               int P, int G, int C, long long rows, float eps, void* stream) {
  if (!partial || !w || !b || !scale || !shift) return SFM_ERR_ARG;
  if (B <= 0 || P <= 0 || G <= 0 || C % G != 0) return SFM_ERR_SHAPE;
  double count = (double)rows * (double)(C / G);
  SFM_LAUNCH(gn_finalize_kernel, dim3(G, B), dim3(64), 0, (hipStream_t)stream, partial, w, b, scale, shift, P,
                     G, C, count, eps);
  return SFM_OK;
}

template <class T>
__device__ __forceinline__ void load8(const void* p, int is_f32, long long idx, float* v) {
  if (is_f32) {
    const f32x4* q = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + idx);
    f32x4 a = q[0], c = q[1];
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = c[0]; v[5] = c[1]; v[6] = c[2]; v[7] = c[3];
  } else {
    u32x4 a = *reinterpret_cast<const u32x4*>(reinterpret_cast<const u16*>(p) + idx);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = T::to_f32((u16)(a[i] & 0xffffu));
      v[2 * i + 1] = T::to_f32((u16)(a[i] >> 16));
    }
  }
}

template <class T>
__device__ __forceinline__ void store8(void* p, int is_f32, long long idx, const float* v) {
  if (is_f32) {
    f32x4* q = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + idx);
    f32x4 a = {v[0], v[1], v[2], v[3]}, c = {v[4], v[5], v[6], v[7]};
    q[0] = a;
    q[1] = c;
  } else {
    u32x4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = pack2<T>(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<u32x4*>(reinterpret_cast<u16*>(p) + idx) = a;
  }
}

// y[b,l,c] = act( x1*sc1+sh1 (+ x2*sc2+sh2) ), channels-last, 8 channels per thread
template <class T>
__global__ __launch_bounds__(256) void gn_apply_kernel(const void* x1, const float* __restrict__ sc1,
                                                       const float* __restrict__ sh1, const void* x2,
                                                       const float* __restrict__ sc2, const float* __restrict__ sh2,
                                                       void* out, long long rows_per_batch, int C, long long total8,
                                                       int in_f32, int out_f32, int act) {
  const int cpr = C >> 3;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total8; e += (long long)gridDim.x * 256) {
    long long row = e / cpr;
    int c0 = (int)(e - row * cpr) * 8;
    long long b = row / rows_per_batch;
    float v[8], u[8];
    load8<T>(x1, in_f32, e * 8, v);
    const float* s1 = sc1 + b * C + c0;
    const float* h1 = sh1 + b * C + c0;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = v[i] * s1[i] + h1[i];
    if (x2) {
      load8<T>(x2, in_f32, e * 8, u);
      const float* s2 = sc2 + b * C + c0;
      const float* h2 = sh2 + b * C + c0;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += u[i] * s2[i] + h2[i];
    }
    if (act == 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = gelu_erf(v[i]);
    } else if (act == 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = swish_f(v[i]);
    }
    store8<T>(out, out_f32, e * 8, v);
  }
}

// The same pass for C a power of two in [64, 2048] (every caller on the path): grid (row tiles, B), block 256 = (C/8 channel
// vectors) x (2048/C row lanes); a thread keeps the scale / shift of ITS 8 channels in registers and walks down the rows (the
// kernel above divides a 64-bit element index twice and re-reads 16 coefficients per 8 elements, and its erff is ~35 instructions:
// VALU-bound at 3.9 TB/s on the training step's nodes).  GELU with a 16-bit result = z * normal_cdf_poly(z) (no transcendental,
// |error| < 5.7e-5 |z|); an fp32 result keeps erff.
template <class T, int ACT, bool TWO>
__global__ __launch_bounds__(256) void gn_apply_rows_kernel(const void* __restrict__ x1, const float* __restrict__ sc1,
                                                            const float* __restrict__ sh1, const void* __restrict__ x2,
                                                            const float* __restrict__ sc2, const float* __restrict__ sh2,
                                                            void* __restrict__ out, int L, int C, int in_f32, int out_f32,
                                                            int rows_per_block) {
  const long long b = blockIdx.y;
  const int nv = C >> 3, rl = 256 / nv;
  const int tv = threadIdx.x % nv, tr = threadIdx.x / nv, c0 = tv * 8;
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  float s1[8], h1[8], s2[8];                          // h1: both shifts
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s1[i] = sc1[b * C + c0 + i];
    h1[i] = sh1[b * C + c0 + i];
    if (TWO) { s2[i] = sc2[b * C + c0 + i]; h1[i] += sh2[b * C + c0 + i]; }
  }
  for (int l = l0 + tr; l < l1; l += rl) {
    const long long e = (b * L + l) * C + c0;
    float v[8], u[8];
    load8<T>(x1, in_f32, e, v);
    if (TWO) load8<T>(x2, in_f32, e, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float y = fmaf(v[i], s1[i], h1[i]);
      if (TWO) y = fmaf(u[i], s2[i], y);
      // 16-bit result: z * Phi(z) with the polynomial CDF (|error| < 5.7e-5 inside its range) - outside |z| <= 3.75 the
      // polynomial is clamped (a negative tail -5e-5 |z| where exact GELU goes to 0): those lanes take the erf form
      if (ACT == 1) y = (out_f32 || fabsf(y) > 3.75f) ? gelu_erf(y) : y * normal_cdf_poly(y);
      else if (ACT == 2) y = swish_f(y);
      v[i] = y;
    }
    store8<T>(out, out_f32, e, v);
  }
}

extern "C" int sfm_gn_apply(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2,
                            const float* sh2, void* out, int B, long long rows_per_batch, int C, int in_f32, int out_f32,
                            int act, int dtype, void* stream) {
  if (!x1 || !sc1 || !sh1 || !out) return SFM_ERR_ARG;
  if (C % 8 != 0 || B <= 0 || rows_per_batch <= 0) return SFM_ERR_SHAPE;
  if (C >= 64 && C <= 2048 && (C & (C - 1)) == 0 && B <= 65535 && rows_per_batch < (1ll << 31) && act >= 0 && act <= 2) {
    const int L = (int)rows_per_batch;
    const int rpb = 8 * (2048 / C) > 256 ? 8 * (2048 / C) : 256;
    dim3 grid((L + rpb - 1) / rpb, B), block(256);
    hipStream_t st = (hipStream_t)stream;
#define GNA_GO(T, A, W) SFM_LAUNCH((gn_apply_rows_kernel<T, A, W>), grid, block, 0, st, x1, sc1, sh1, x2, sc2, sh2, out, L, C, in_f32, out_f32, rpb)
#define GNA_A(T, A) do { if (x2) GNA_GO(T, A, true); else GNA_GO(T, A, false); } while (0)
#define GNA_T(T) do { if (act == 1) GNA_A(T, 1); else if (act == 2) GNA_A(T, 2); else GNA_A(T, 0); } while (0)
    if (dtype == SFM_DT_F16) GNA_T(F16); else GNA_T(BF16);
#undef GNA_T
#undef GNA_A
#undef GNA_GO
    return SFM_OK;
  }
  long long total8 = (long long)B * rows_per_batch * (C / 8);
  long long nb = (total8 + 255) / 256;
  if (nb > 16384) nb = 16384;
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((gn_apply_kernel<F16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x1, sc1, sh1, x2,
                       sc2, sh2, out, rows_per_batch, C, total8, in_f32, out_f32, act);
  else
    SFM_LAUNCH((gn_apply_kernel<BF16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x1, sc1, sh1,
                       x2, sc2, sh2, out, rows_per_batch, C, total8, in_f32, out_f32, act);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// Depthwise Conv1d(k, pad (k-1)/2, groups=C) + BatchNorm1d(eval) + Swish on a
// channels-last [B, T, C] 16-bit tensor (models/conformer.py:117-119).
// Tile = 64 frames (+ k-1 halo) x C channels in LDS; each work item computes
// 4 consecutive frames of one channel pair with a sliding weight window.
// ---------------------------------------------------------------------------
static_assert(SFM_DWCONV_TILE == 64, "frames of a workgroup of the register-resident depthwise kernels");
template <class T>
__global__ __launch_bounds__(256) void dwconv_bn_swish_kernel(const u16* __restrict__ x, const float* __restrict__ wdw,
                                                              const float* __restrict__ bdw, const float* __restrict__ bnw,
                                                              const float* __restrict__ bnb, const float* __restrict__ bnm,
                                                              const float* __restrict__ bnv, u16* __restrict__ out,
                                                              int Tlen, int C, int KS, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int halo = KS - 1, padl = (KS - 1) / 2;
  const int rows = SFM_DWCONV_TILE + halo;
  u16* xs = reinterpret_cast<u16*>(dsm);                                 // [rows][C]
  float* ws = reinterpret_cast<float*>(dsm + (((size_t)rows * C * 2 + 15) & ~(size_t)15));  // [KS][C]
  float* scs = ws + (size_t)KS * C;                                      // [C] scale
  float* shs = scs + C;                                                  // [C] shift (conv bias folded)
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * SFM_DWCONV_TILE;
  const int b = blockIdx.y;
  const u16* xb = x + (long long)b * Tlen * C;
  const int cpr = C >> 3;
  for (int e = tid; e < rows * cpr; e += 256) {
    int r = e / cpr, c8 = (e - r * cpr) * 8;
    int t = t0 - padl + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (t >= 0 && t < Tlen) v = *reinterpret_cast<const u32x4*>(xb + (long long)t * C + c8);
    *reinterpret_cast<u32x4*>(&xs[r * C + c8]) = v;
  }
  for (int e = tid; e < KS * C; e += 256) {
    int k = e / C, c = e - k * C;
    ws[e] = wdw[c * KS + k];
  }
  for (int c = tid; c < C; c += 256) {
    float sc = bnw[c] * rsqrtf(bnv[c] + eps);
    scs[c] = sc;
    shs[c] = bnb[c] - bnm[c] * sc + bdw[c] * sc;
  }
  __syncthreads();
  const int npair = C >> 1;
  const int items = (SFM_DWCONV_TILE / 4) * npair;
  u16* ob = out + (long long)b * Tlen * C;
  for (int it = tid; it < items; it += 256) {
    int pair = it % npair, tq = it / npair;
    int c = pair * 2, tl = tq * 4;
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
    float w0[4] = {0.f, 0.f, 0.f, 0.f}, w1[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < KS + 3; ++k) {
      // shift the weight window: w[o] = W[k - o]
      w0[3] = w0[2]; w0[2] = w0[1]; w0[1] = w0[0];
      w1[3] = w1[2]; w1[2] = w1[1]; w1[1] = w1[0];
      if (k < KS) {
        w0[0] = ws[k * C + c];
        w1[0] = ws[k * C + c + 1];
      } else {
        w0[0] = 0.f;
        w1[0] = 0.f;
      }
      uint32_t pk = *reinterpret_cast<const uint32_t*>(&xs[(tl + k) * C + c]);
      float x0 = T::to_f32((u16)(pk & 0xffffu)), x1 = T::to_f32((u16)(pk >> 16));
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        a0[o] += w0[o] * x0;
        a1[o] += w1[o] * x1;
      }
    }
    float s0 = scs[c], s1 = scs[c + 1], h0 = shs[c], h1 = shs[c + 1];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      int t = t0 + tl + o;
      if (t < Tlen) {
        float y0 = swish_f(a0[o] * s0 + h0), y1 = swish_f(a1[o] * s1 + h1);
        *reinterpret_cast<uint32_t*>(&ob[(long long)t * C + c]) = pack2<T>(y0, y1);
      }
    }
  }
}

// Register-weight variant for the shapes of the path (KS = 31 or 7, C/2 | 256): the 2*KS taps of a
// thread's channel pair live in registers, LDS holds only the 16-bit input tile (3 workgroups per CU),
// weights arrive pre-transposed [KS][C] with BatchNorm folded into per-channel scale/shift.
// VARLEN: the packed form.  x / out hold the rows of all utterances back to back (utterance u = rows [frame_off[u],
// frame_off[u + 1])); workgroup i takes entry i of the tile table (utterance, 64-frame tile of that utterance) the host built
// from the lengths (ops.dwconv_tiles), so tiles start at the utterance's first frame and the zero edge is the utterance's own.
template <class T, int KS, bool VARLEN = false>
__global__ __launch_bounds__(256) void dwconv_reg_kernel(const u16* __restrict__ x, const float* __restrict__ wT,
                                                         const float* __restrict__ sc, const float* __restrict__ sh,
                                                         void* __restrict__ out, int Tlen, int C, int act, int out_f32,
                                                         const int* __restrict__ frame_off = nullptr,
                                                         const int* __restrict__ tiles = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  u16* xs = reinterpret_cast<u16*>(dsm);                                 // [SFM_DWCONV_TILE + KS - 1][C]
  constexpr int padl = (KS - 1) / 2, rows = SFM_DWCONV_TILE + KS - 1;
  const int tid = threadIdx.x;
  int t0 = blockIdx.x * SFM_DWCONV_TILE;
  long long row0 = (long long)blockIdx.y * Tlen;                         // first row of the utterance
  if (VARLEN) {
    const int u = tiles[2 * blockIdx.x];
    t0 = tiles[2 * blockIdx.x + 1] * SFM_DWCONV_TILE;
    row0 = frame_off[u];
    Tlen = frame_off[u + 1] - (int)row0;
  }
  const u16* xb = x + row0 * C;
  const int cpr = C >> 3;
  for (int e = tid; e < rows * cpr; e += 256) {
    const int r = e / cpr, c8 = (e - r * cpr) * 8;
    const int t = t0 - padl + r;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (t >= 0 && t < Tlen) v = *reinterpret_cast<const u32x4*>(xb + (long long)t * C + c8);
    *reinterpret_cast<u32x4*>(&xs[r * C + c8]) = v;
  }
  const int npair = C >> 1;
  const int p = tid % npair, grp = tid / npair, ngrp = 256 / npair;
  const int c = 2 * p;
  float w0[KS], w1[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) {
    const f32x2 w = *reinterpret_cast<const f32x2*>(wT + k * C + c);
    w0[k] = w[0];
    w1[k] = w[1];
  }
  const float s0 = sc[c], s1 = sc[c + 1], h0 = sh[c], h1 = sh[c + 1];
  __syncthreads();
  const long long obase = row0 * C;
  const int per = SFM_DWCONV_TILE / ngrp;                                          // frames per thread (multiple of 4)
  for (int tl = grp * per; tl < (grp + 1) * per; tl += 4) {
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KS + 3; ++k) {
      const uint32_t pk = *reinterpret_cast<const uint32_t*>(&xs[(tl + k) * C + c]);
      const float x0 = T::to_f32((u16)(pk & 0xffffu)), x1 = T::to_f32((u16)(pk >> 16));
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int kk = k - o;                                            // compile-time after unrolling
        if (kk >= 0 && kk < KS) {
          a0[o] += w0[kk] * x0;
          a1[o] += w1[kk] * x1;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int t = t0 + tl + o;
      if (t < Tlen) {
        float y0 = a0[o] * s0 + h0, y1 = a1[o] * s1 + h1;
        if (act) { y0 = swish_f(y0); y1 = swish_f(y1); }
        const long long off = obase + (long long)t * C + c;
        if (out_f32) {
          f32x2 w = {y0, y1};
          *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(out) + off) = w;
        } else {
          *reinterpret_cast<uint32_t*>(reinterpret_cast<u16*>(out) + off) = pack2<T>(y0, y1);
        }
      }
    }
  }
}

// fp16 form of the kernel above (KS odd): the taps are summed two at a time with v_dot2_f32_f16 - (w[2j], w[2j+1]) . (x[t+2j], x[t+2j+1]),
// fp32 accumulation, products of two fp16 values are exact in fp32 - instead of one v_fma_f32 per tap after two converts per input
// value.  The time pairs of a channel are built from the staged channels-last rows with one v_perm_b32 each (even pairs for the
// even outputs of a step, odd pairs for the odd ones): per 4 outputs x 2 channels 128 dot products + 68 permutes against 248
// multiply-adds + 68 converts.  New rounding: the taps, once, to fp16 (the operand format of every MFMA of the path).
typedef _Float16 dw_h2 __attribute__((ext_vector_type(2)));
template <int KS, bool VARLEN = false>                                   // VARLEN: the packed form, as in dwconv_reg_kernel
__global__ __launch_bounds__(256) void dwconv_dot_kernel(const u16* __restrict__ x, const float* __restrict__ wT,
                                                         const float* __restrict__ sc, const float* __restrict__ sh,
                                                         void* __restrict__ out, int Tlen, int C, int act, int out_f32,
                                                         const int* __restrict__ frame_off = nullptr,
                                                         const int* __restrict__ tiles = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  u16* xs = reinterpret_cast<u16*>(dsm);                                 // [SFM_DWCONV_TILE + KS - 1][C]
  constexpr int padl = (KS - 1) / 2, rows = SFM_DWCONV_TILE + KS - 1;
  constexpr int NP = (KS + 1) / 2;                                       // tap pairs (the last one = (w[KS-1], 0))
  constexpr int NR = KS + 3;                                             // staged rows a step of 4 outputs reads
  const int tid = threadIdx.x;
  int t0 = blockIdx.x * SFM_DWCONV_TILE;
  long long row0 = (long long)blockIdx.y * Tlen;                         // first row of the utterance
  if (VARLEN) {
    const int u = tiles[2 * blockIdx.x];
    t0 = tiles[2 * blockIdx.x + 1] * SFM_DWCONV_TILE;
    row0 = frame_off[u];
    Tlen = frame_off[u + 1] - (int)row0;
  }
  const u16* xb = x + row0 * C;
  const int cpr = C >> 3;
  // staging in batches of 12 chunks per thread with ALL of a batch's loads issued before its first LDS write (the rolled
  // load -> write loop of the kernel above pays one memory round trip per 16 bytes: 12 in a row at C = 256, and that latency
  // chain, not the arithmetic, is most of a workgroup's life)
  for (int e0 = tid; e0 < rows * cpr; e0 += 256 * 12) {
    u32x4 v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int e = e0 + 256 * i;
      const int r = e / cpr, c8 = (e - r * cpr) * 8;
      const int t = t0 - padl + r;
      v[i] = u32x4{0u, 0u, 0u, 0u};
      if (e < rows * cpr && t >= 0 && t < Tlen) v[i] = *reinterpret_cast<const u32x4*>(xb + (long long)t * C + c8);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int e = e0 + 256 * i;
      const int r = e / cpr, c8 = (e - r * cpr) * 8;
      if (e < rows * cpr) *reinterpret_cast<u32x4*>(&xs[r * C + c8]) = v[i];
    }
  }
  const int npair = C >> 1;
  const int p = tid % npair, grp = tid / npair, ngrp = 256 / npair;
  const int c = 2 * p;
  dw_h2 w0[NP], w1[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const f32x2 a = *reinterpret_cast<const f32x2*>(wT + (2 * j) * C + c);
    f32x2 bq = {0.f, 0.f};
    if (2 * j + 1 < KS) bq = *reinterpret_cast<const f32x2*>(wT + (2 * j + 1) * C + c);
    w0[j] = dw_h2{(_Float16)a[0], (_Float16)bq[0]};
    w1[j] = dw_h2{(_Float16)a[1], (_Float16)bq[1]};
  }
  const float s0 = sc[c], s1 = sc[c + 1], h0 = sh[c], h1 = sh[c + 1];
  __syncthreads();
  const long long obase = row0 * C;
  const int per = SFM_DWCONV_TILE / ngrp;                                          // frames per thread (multiple of 4)
  for (int tl = grp * per; tl < (grp + 1) * per; tl += 4) {
    uint32_t d[NR + 1];                                                  // row k of the step: (x[k][c], x[k][c + 1])
#pragma unroll
    for (int k = 0; k < NR; ++k) d[k] = *reinterpret_cast<const uint32_t*>(&xs[(tl + k) * C + c]);
    d[NR] = d[NR - 1];                                                   // (multiplied by the zero of the last tap pair)
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        // time pair (x[o + 2j], x[o + 2j + 1]) of each channel: the low / high halves of two staged rows
        const uint32_t lo = __builtin_amdgcn_perm(d[o + 2 * j + 1], d[o + 2 * j], 0x05040100u);
        const uint32_t hi = __builtin_amdgcn_perm(d[o + 2 * j + 1], d[o + 2 * j], 0x07060302u);
        a0[o] = __builtin_amdgcn_fdot2(w0[j], __builtin_bit_cast(dw_h2, lo), a0[o], false);
        a1[o] = __builtin_amdgcn_fdot2(w1[j], __builtin_bit_cast(dw_h2, hi), a1[o], false);
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int t = t0 + tl + o;
      if (t < Tlen) {
        float y0 = a0[o] * s0 + h0, y1 = a1[o] * s1 + h1;
        if (act) { y0 = swish_f(y0); y1 = swish_f(y1); }
        const long long off = obase + (long long)t * C + c;
        if (out_f32) {
          f32x2 w = {y0, y1};
          *reinterpret_cast<f32x2*>(reinterpret_cast<float*>(out) + off) = w;
        } else {
          *reinterpret_cast<uint32_t*>(reinterpret_cast<u16*>(out) + off) = pack2<F16>(y0, y1);
        }
      }
    }
  }
}

// (the launchers' VARLEN form: B = 0 rows of the grid's second dimension are replaced by the n_tiles entries of `tiles`)
template <int KS, bool VARLEN = false>
static int launch_dwconv_dot(const void* x, const float* wT, const float* sc, const float* sh, void* out, int B, int Tn,
                             int C, int act, int out_f32, hipStream_t st, const int* frame_off = nullptr,
                             const int* tiles = nullptr, int n_tiles = 0) {
  const int lds = (SFM_DWCONV_TILE + KS - 1) * C * 2;                  // grows with C: the grant follows the widest launch so far
  const dim3 grid = VARLEN ? dim3(n_tiles, 1) : dim3((Tn + SFM_DWCONV_TILE - 1) / SFM_DWCONV_TILE, B);
  SFM_LAUNCH_LDS((dwconv_dot_kernel<KS, VARLEN>), grid, dim3(256), lds, st, (const u16*)x, wT, sc, sh, out, Tn, C, act, out_f32,
                 frame_off, tiles);
  return SFM_OK;
}

template <class T, int KS, bool VARLEN = false>
static int launch_dwconv_reg(const void* x, const float* wT, const float* sc, const float* sh, void* out, int B, int Tn,
                             int C, int act, int out_f32, hipStream_t st, const int* frame_off = nullptr,
                             const int* tiles = nullptr, int n_tiles = 0) {
  const int lds = (SFM_DWCONV_TILE + KS - 1) * C * 2;                  // as above
  const dim3 grid = VARLEN ? dim3(n_tiles, 1) : dim3((Tn + SFM_DWCONV_TILE - 1) / SFM_DWCONV_TILE, B);
  SFM_LAUNCH_LDS((dwconv_reg_kernel<T, KS, VARLEN>), grid, dim3(256), lds, st, (const u16*)x, wT, sc, sh, out, Tn, C, act, out_f32,
                 frame_off, tiles);
  return SFM_OK;
}

// Any channel count and any odd KS (the shapes the register-resident kernels do not take, e.g. the training-mode
// ConvolutionModule at C 192 / 384): one output element per thread, taps and scale / shift read from global memory.
// VARLEN: the packed form; each element finds its utterance by a binary search in frame_off [nutt + 1].
template <class T, bool VARLEN = false>
__global__ __launch_bounds__(256) void dwconv_generic_kernel(const u16* __restrict__ x, const float* __restrict__ wT,
                                                             const float* __restrict__ sc, const float* __restrict__ sh,
                                                             void* __restrict__ out, int Tlen, int C, int KS, long long total,
                                                             int act, int out_f32, const int* __restrict__ frame_off = nullptr,
                                                             int nutt = 0) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long long bt = i / C;                                            // b * Tlen + t (packed form: the packed row)
  int t;
  if (VARLEN) {
    const int u = sfm_seg_find(frame_off, nutt, (int)bt);
    t = (int)bt - frame_off[u];
    Tlen = frame_off[u + 1] - frame_off[u];
  } else {
    t = (int)(bt % Tlen);
  }
  const u16* xc = x + (bt - t) * C + c;                                  // (b, 0, c)
  const int padl = (KS - 1) / 2;
  float acc = 0.f;
  for (int k = 0; k < KS; ++k) {
    const int tt = t + k - padl;
    if (tt >= 0 && tt < Tlen) acc += wT[(long long)k * C + c] * T::to_f32(xc[(long long)tt * C]);
  }
  float y = acc * sc[c] + sh[c];
  if (act) y = swish_f(y);
  if (out_f32) reinterpret_cast<float*>(out)[i] = y;
  else reinterpret_cast<u16*>(out)[i] = T::from_f32(y);
}

// KS 7 / 31 with C in {32, 64, 128, 256, 512}: the shapes of the register-resident kernels
static bool dwconv_reg_shape(int C, int KS) {
  return (KS == 7 || KS == 31) && C % 8 == 0 && C <= 512 && (256 % (C / 2)) == 0 && (SFM_DWCONV_TILE / (256 / (C / 2))) % 4 == 0;
}

// The routing of sfm_dwconv_folded and of its packed form (VARLEN: Tn = 0, rows = sum_T, B utterances in frame_off): the
// register-resident kernels on their shapes, the generic kernel on everything else.
template <bool VARLEN>
static int dwconv_folded_route(const void* x, const float* wT, const float* sc, const float* sh, void* out, int B, int Tn,
                               long long rows, int C, int KS, int act, int out_f32, int dtype, hipStream_t st,
                               const int* frame_off, const int* tiles, int n_tiles) {
  if (!dwconv_reg_shape(C, KS)) {
    const long long total = rows * C;
    const long long nb = (total + 255) / 256;
    if (nb > 0x7fffffffLL) return SFM_ERR_SHAPE;
    if (dtype == SFM_DT_F16)
      SFM_LAUNCH((dwconv_generic_kernel<F16, VARLEN>), dim3((unsigned)nb), dim3(256), 0, st, (const u16*)x, wT, sc, sh, out, Tn, C, KS,
                 total, act, out_f32, frame_off, VARLEN ? B : 0);
    else
      SFM_LAUNCH((dwconv_generic_kernel<BF16, VARLEN>), dim3((unsigned)nb), dim3(256), 0, st, (const u16*)x, wT, sc, sh, out, Tn, C, KS,
                 total, act, out_f32, frame_off, VARLEN ? B : 0);
    return SFM_OK;
  }
  // KS 31: fp16 with a 16-bit output on the dot-product form (its taps are rounded to fp16: 2^-12 of a tap, under the rounding of
  // the output), everything else on the multiply-add kernel with fp32 taps - the fp32 output of the training forward, which
  // feeds the BatchNorm statistics, would carry the tap rounding as its largest error (2e-4 of the output against 3e-7)
#define DW_GO(L) return L(x, wT, sc, sh, out, B, Tn, C, act, out_f32, st, frame_off, tiles, n_tiles)
  if (KS == 31) {
    if (dtype == SFM_DT_F16 && !out_f32) DW_GO((launch_dwconv_dot<31, VARLEN>));
    if (dtype == SFM_DT_F16) DW_GO((launch_dwconv_reg<F16, 31, VARLEN>));
    DW_GO((launch_dwconv_reg<BF16, 31, VARLEN>));
  }
  if (dtype == SFM_DT_F16) DW_GO((launch_dwconv_reg<F16, 7, VARLEN>));
  DW_GO((launch_dwconv_reg<BF16, 7, VARLEN>));
#undef DW_GO
}

// wT [KS][C] fp32 (transposed depthwise weights), sc/sh [C] = BatchNorm(eval) folded with the conv bias:
// y = act ? swish(conv(x) * sc + sh) : conv(x) * sc + sh ; 16-bit or fp32 output.  KS odd; KS 7 / 31 with C in
// {32, 64, 128, 256, 512} on the register-resident kernels, everything else on the generic one.
extern "C" int sfm_dwconv_folded(const void* x, const float* wT, const float* sc, const float* sh, void* out, int B, int T,
                                 int C, int KS, int act, int out_f32, int dtype, void* stream) {
  if (!x || !wT || !sc || !sh || !out) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || C <= 0 || KS < 1 || (KS & 1) == 0) return SFM_ERR_SHAPE;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  return dwconv_folded_route<false>(x, wT, sc, sh, out, B, T, (long long)B * T, C, KS, act, out_f32, dtype, (hipStream_t)stream,
                                    nullptr, nullptr, 0);
}

// Packed (variable-length) form of sfm_dwconv_folded: x / out [sum_T, C] hold B utterances back to back, utterance u = rows
// [frame_off[u], frame_off[u + 1]) (int32[B + 1] on the device), each convolved with a zero edge at its own first and last frame.
// The register-resident kernels take one workgroup per entry of `tiles` (int32[n_tiles][2] = utterance, 64-frame tile of that
// utterance: every tile of every utterance once), the generic kernel does not read the table.
extern "C" int sfm_dwconv_folded_varlen(const void* x, const float* wT, const float* sc, const float* sh, void* out,
                                        const int* frame_off, const int* tiles, int n_tiles, int B, int max_T, int sum_T, int C,
                                        int KS, int act, int out_f32, int dtype, void* stream) {
  if (!x || !wT || !sc || !sh || !out || !frame_off) return SFM_ERR_ARG;
  if (B <= 0 || max_T <= 0 || sum_T < max_T || C <= 0 || KS < 1 || (KS & 1) == 0) return SFM_ERR_SHAPE;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  if (dwconv_reg_shape(C, KS)) {                               // (only these kernels read the tile table)
    if (!tiles) return SFM_ERR_ARG;
    if (n_tiles < B || (long long)n_tiles > (long long)B * ((max_T + SFM_DWCONV_TILE - 1) / SFM_DWCONV_TILE)) return SFM_ERR_SHAPE;
  }
  return dwconv_folded_route<true>(x, wT, sc, sh, out, B, 0, sum_T, C, KS, act, out_f32, dtype, (hipStream_t)stream, frame_off,
                                   tiles, n_tiles);
}

extern "C" int sfm_dwconv_bn_swish(const void* x, const float* wdw, const float* bdw, const float* bnw,
                                   const float* bnb, const float* bnm, const float* bnv, void* out, int B, int T,
                                   int C, int KS, float eps, int dtype, void* stream) {
  if (!x || !wdw || !bdw || !bnw || !bnb || !bnm || !bnv || !out) return SFM_ERR_ARG;
  if (C % 8 != 0 || KS < 1 || (KS & 1) == 0 || B <= 0 || T <= 0) return SFM_ERR_SHAPE;
  size_t rows = SFM_DWCONV_TILE + KS - 1;
  size_t lds_sz = ((rows * C * 2 + 15) & ~(size_t)15) + ((size_t)KS * C + 2 * (size_t)C) * 4;
  if (lds_sz > 160 * 1024) return SFM_ERR_SHAPE;
  const int lds = (int)lds_sz;
  dim3 grid((T + SFM_DWCONV_TILE - 1) / SFM_DWCONV_TILE, B), block(256);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH_LDS((dwconv_bn_swish_kernel<F16>), grid, block, lds, (hipStream_t)stream, (const u16*)x, wdw, bdw,
                   bnw, bnb, bnm, bnv, (u16*)out, T, C, KS, eps);
  else
    SFM_LAUNCH_LDS((dwconv_bn_swish_kernel<BF16>), grid, block, lds, (hipStream_t)stream, (const u16*)x, wdw, bdw,
                   bnw, bnb, bnm, bnv, (u16*)out, T, C, KS, eps);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// Layout / packing kernels
// ---------------------------------------------------------------------------
// fp32 [M, C] (row stride lds_) -> 16-bit [M, ldd] at column offset; cols [C, Cz) zero-filled
template <class T>
__global__ __launch_bounds__(256) void convert_rows_kernel(const float* __restrict__ src, u16* __restrict__ dst,
                                                           long long M, int C, int Cz, long long lds_, long long ldd) {
  long long total = M * Cz;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    long long m = e / Cz;
    int c = (int)(e - m * Cz);
    float v = (c < C) ? src[m * lds_ + c] : 0.f;
    dst[m * ldd + c] = T::from_f32(v);
  }
}

// 8 columns per thread: two 16-byte loads, one 16-byte store, 32-bit index arithmetic (the scalar kernel above divides a
// 64-bit index per ELEMENT and stores 2 bytes at a time: 2.9 TB/s on the training step's [205 056, 256] conversions)
template <class T>
__global__ __launch_bounds__(256) void convert_rows_vec_kernel(const float* __restrict__ src, u16* __restrict__ dst, int M, int C,
                                                               int cpr, long long lds_, long long ldd) {
  const int total = M * cpr;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int m = e / cpr, c = (e - m * cpr) * 8;
    u32x4 o = {0u, 0u, 0u, 0u};
    if (c < C) {                                          // (C % 8 == 0: a chunk is whole or all padding)
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + m * lds_ + c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(src + m * lds_ + c + 4);
      o = u32x4{pack2<T>(a[0], a[1]), pack2<T>(a[2], a[3]), pack2<T>(b[0], b[1]), pack2<T>(b[2], b[3])};
    }
    *reinterpret_cast<u32x4*>(dst + m * ldd + c) = o;
  }
}

extern "C" int sfm_convert_rows(const float* src, void* dst, long long M, int C, int Cz, long long ld_src,
                                long long ld_dst, int dtype, void* stream) {
  if (!src || !dst) return SFM_ERR_ARG;
  if (M <= 0 || C <= 0 || Cz < C) return SFM_ERR_SHAPE;
  if (C % 8 == 0 && Cz % 8 == 0 && ld_src % 4 == 0 && ld_dst % 8 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0 &&
      M * (long long)(Cz / 8) < (1ll << 31)) {
    const int cpr = Cz / 8;
    long long nbv = (M * cpr + 255) / 256;
    if (nbv > 32768) nbv = 32768;
    if (dtype == SFM_DT_F16)
      SFM_LAUNCH((convert_rows_vec_kernel<F16>), dim3((unsigned)nbv), dim3(256), 0, (hipStream_t)stream, src, (u16*)dst, (int)M, C, cpr,
                 ld_src, ld_dst);
    else
      SFM_LAUNCH((convert_rows_vec_kernel<BF16>), dim3((unsigned)nbv), dim3(256), 0, (hipStream_t)stream, src, (u16*)dst, (int)M, C, cpr,
                 ld_src, ld_dst);
    return SFM_OK;
  }
  long long nb = (M * Cz + 255) / 256;
  if (nb > 16384) nb = 16384;
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((convert_rows_kernel<F16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src,
                       (u16*)dst, M, C, Cz, ld_src, ld_dst);
  else
    SFM_LAUNCH((convert_rows_kernel<BF16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, src,
                       (u16*)dst, M, C, Cz, ld_src, ld_dst);
  return SFM_OK;
}

// transpose [B, R, Ccols] <-> [B, Ccols, R] through a 32x33 LDS tile.
// src element (b, r, c) at src[b*sb + r*sr + c]; dst element at dst[b*db + c*dc + r].
// src fp32 or 16-bit; dst fp32 or 16-bit.
template <class T>
__global__ __launch_bounds__(256) void transpose_kernel(const void* src, void* dst, int R, int Cc, long long sb,
                                                        long long sr, long long db, long long dc, int src_f32,
                                                        int dst_f32) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    int r = r0 + i, c = c0 + tx;
    float v = 0.f;
    if (r < R && c < Cc) {
      long long idx = (long long)b * sb + (long long)r * sr + c;
      v = src_f32 ? reinterpret_cast<const float*>(src)[idx] : T::to_f32(reinterpret_cast<const u16*>(src)[idx]);
    }
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    int c = c0 + i, r = r0 + tx;
    if (r < R && c < Cc) {
      long long idx = (long long)b * db + (long long)c * dc + r;
      float v = tile[tx][i];
      if (dst_f32) reinterpret_cast<float*>(dst)[idx] = v;
      else reinterpret_cast<u16*>(dst)[idx] = T::from_f32(v);
    }
  }
}

extern "C" int sfm_transpose(const void* src, void* dst, int B, int R, int C, long long src_batch, long long src_row,
                             long long dst_batch, long long dst_row, int src_f32, int dst_f32, int dtype, void* stream) {
  if (!src || !dst) return SFM_ERR_ARG;
  if (B <= 0 || R <= 0 || C <= 0) return SFM_ERR_SHAPE;
  dim3 grid((C + 31) / 32, (R + 31) / 32, B), block(256);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((transpose_kernel<F16>), grid, block, 0, (hipStream_t)stream, src, dst, R, C, src_batch, src_row,
                       dst_batch, dst_row, src_f32, dst_f32);
  else
    SFM_LAUNCH((transpose_kernel<BF16>), grid, block, 0, (hipStream_t)stream, src, dst, R, C, src_batch,
                       src_row, dst_batch, dst_row, src_f32, dst_f32);
  return SFM_OK;
}

// adaptive average pool along time (glue G1): src fp32 [B, Tin, ld_src] cols [0,C)
// -> dst 16-bit [B, Tout, ld_dst] cols [0, C).  window i = [floor(i*Tin/Tout), ceil((i+1)*Tin/Tout))
template <class T, int SRC>                            // SRC: 0 fp32, 1 fp16, 2 bf16 source
__global__ __launch_bounds__(256) void pool_time_kernel(const void* __restrict__ src_, u16* dst16, float* dst32,
                                                        int Tin, int Tout, int C, long long ld_src, long long ld_dst,
                                                        const float* __restrict__ scale, const float* __restrict__ shift) {
  const int b = blockIdx.z, i = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  long long s = ((long long)i * Tin) / Tout;
  long long e = (((long long)(i + 1)) * Tin + Tout - 1) / Tout;
  float acc = 0.f;
  for (long long t = s; t < e; ++t) {
    const long long o = ((long long)b * Tin + t) * ld_src + c;
    if (SRC == 0) acc += reinterpret_cast<const float*>(src_)[o];
    else if (SRC == 1) acc += F16::to_f32(reinterpret_cast<const u16*>(src_)[o]);
    else acc += BF16::to_f32(reinterpret_cast<const u16*>(src_)[o]);
  }
  acc /= (float)(e - s);
  if (scale) acc = acc * scale[(long long)b * C + c] + shift[(long long)b * C + c];   // affine commutes with the average
  long long o = ((long long)b * Tout + i) * ld_dst + c;
  if (dst16) dst16[o] = T::from_f32(acc);
  if (dst32) dst32[o] = acc;
}

// 8 channels per thread (16-byte loads of a 16-bit source, 2 x 16 bytes of an fp32 one): a 256-thread workgroup covers (256 / (C / 8)) output frames of one utterance; needs C % 8 == 0, C / 8 a divisor of 256 and
// 16-byte aligned rows.  The scalar kernel above moved 2 or 4 bytes per lane and was bound by its load count, not by HBM.
template <class T, int SRC, int PG>
__global__ __launch_bounds__(256) void pool_time_vec_kernel(const void* __restrict__ src_, u16* dst16, float* dst32, int Tin, int Tout,
                                                            int C, long long ld_src, long long ld_dst,
                                                            const float* __restrict__ scale, const float* __restrict__ shift) {
  const int tpf = C >> 3;                                  // threads per output frame
  const int fpb = 256 / tpf;                               // output frames per workgroup
  const int b = blockIdx.y;
  const int i = blockIdx.x * fpb + threadIdx.x / tpf;
  const int c = (threadIdx.x % tpf) * 8;
  if (i >= Tout) return;
  // (window bounds in 32-bit arithmetic when the products fit: two emulated 64-bit divisions per thread were a third of this
  //  kernel's instructions; PG == 1: the window is the row itself)
  long long s, e;
  if (PG == 1) { s = i; e = i + 1; }
  else if ((long long)Tin * (Tout + 1) < 2147483647LL) {
    s = (unsigned)(i * Tin) / (unsigned)Tout;
    e = (unsigned)((i + 1) * Tin + Tout - 1) / (unsigned)Tout;
  } else {
    s = ((long long)i * Tin) / Tout;
    e = (((long long)(i + 1)) * Tin + Tout - 1) / Tout;
  }
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // window rows in groups of PG (6; 1 when Tin == Tout: the per-(utterance, channel) affine + convert of already pooled rows) with
  // ALL of a group's loads issued before the first add (a rolled `for t` loop waits out one memory round trip per row; the windows
  // of the path are 5-6 rows: groups of 8 issued 2-3 clamped loads per window for nothing)
  for (long long t0 = s; t0 < e; t0 += PG) {
    if (SRC == 0) {
      f32x4 a0[PG], a1[PG];
#pragma unroll
      for (int k = 0; k < PG; ++k) {
        const long long t = t0 + k < e ? t0 + k : e - 1;     // clamped: loaded, not added
        const long long o = ((long long)b * Tin + t) * ld_src + c;
        a0[k] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(src_) + o);
        a1[k] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(src_) + o + 4);
      }
#pragma unroll
      for (int k = 0; k < PG; ++k)
        if (t0 + k < e) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { acc[j] += a0[k][j]; acc[4 + j] += a1[k][j]; }
        }
    } else {
      u32x4 a[PG];
#pragma unroll
      for (int k = 0; k < PG; ++k) {
        const long long t = t0 + k < e ? t0 + k : e - 1;
        a[k] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const u16*>(src_) + ((long long)b * Tin + t) * ld_src + c);
      }
#pragma unroll
      for (int k = 0; k < PG; ++k)
        if (t0 + k < e) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u16 lo = (u16)(a[k][j] & 0xffffu), hi = (u16)(a[k][j] >> 16);
            acc[2 * j] += SRC == 1 ? F16::to_f32(lo) : BF16::to_f32(lo);
            acc[2 * j + 1] += SRC == 1 ? F16::to_f32(hi) : BF16::to_f32(hi);
          }
        }
    }
  }
  const float inv = 1.0f / (float)(e - s);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] *= inv;
  if (scale) {                                             // affine commutes with the average (16-byte loads: C % 8 == 0, c % 8 == 0)
    const f32x4* sp = reinterpret_cast<const f32x4*>(scale + (long long)b * C + c);
    const f32x4* hp = reinterpret_cast<const f32x4*>(shift + (long long)b * C + c);
    const f32x4 s0 = sp[0], s1 = sp[1], h0 = hp[0], h1 = hp[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = acc[j] * s0[j] + h0[j];
      acc[4 + j] = acc[4 + j] * s1[j] + h1[j];
    }
  }
  const long long o = ((long long)b * Tout + i) * ld_dst + c;
  if (dst16) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pack2<T>(acc[2 * j], acc[2 * j + 1]);
    *reinterpret_cast<u32x4*>(dst16 + o) = w;
  }
  if (dst32) {
    *reinterpret_cast<f32x4*>(dst32 + o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(dst32 + o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  }
}

static int pool_time_go(const void* src, int srcfmt, const float* scale, const float* shift, void* dst16, float* dst32, int B,
                        int Tin, int Tout, int C, long long ld_src, long long ld_dst, int dtype, void* stream) {
  if (!src || (!dst16 && !dst32) || ((scale == nullptr) != (shift == nullptr))) return SFM_ERR_ARG;
  if (B <= 0 || Tin <= 0 || Tout <= 0 || C <= 0) return SFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const int esz = srcfmt == 0 ? 4 : 2;
  const bool vec = (C % 8 == 0) && C <= 2048 && (256 % (C / 8) == 0) && ((ld_src * esz) % 16 == 0) && (((uintptr_t)src) % 16 == 0) &&
                   (!dst16 || ((ld_dst * 2) % 16 == 0 && ((uintptr_t)dst16) % 16 == 0)) &&
                   (!dst32 || ((ld_dst * 4) % 16 == 0 && ((uintptr_t)dst32) % 16 == 0)) &&
                   (!scale || ((((uintptr_t)scale) | ((uintptr_t)shift)) % 16 == 0));
  if (vec) {
    const int fpb = 256 / (C / 8);
    dim3 grid((Tout + fpb - 1) / fpb, B), block(256);
#define POOL_GO(TT, S) do { if (Tin == Tout) SFM_LAUNCH((pool_time_vec_kernel<TT, S, 1>), grid, block, 0, st, src, (u16*)dst16, dst32, Tin, Tout, C, ld_src, ld_dst, scale, shift); \
                            else SFM_LAUNCH((pool_time_vec_kernel<TT, S, 6>), grid, block, 0, st, src, (u16*)dst16, dst32, Tin, Tout, C, ld_src, ld_dst, scale, shift); } while (0)
#define POOL_SRC(TT) { if (srcfmt == 0) POOL_GO(TT, 0); else if (srcfmt == 1) POOL_GO(TT, 1); else POOL_GO(TT, 2); }
    if (dtype == SFM_DT_F16) POOL_SRC(F16) else POOL_SRC(BF16)
#undef POOL_SRC
#undef POOL_GO
    return SFM_OK;
  }
  dim3 grid((C + 255) / 256, Tout, B), block(256);
#define POOL_GO(TT, S) SFM_LAUNCH((pool_time_kernel<TT, S>), grid, block, 0, st, src, (u16*)dst16, dst32, Tin, Tout, C, ld_src, ld_dst, scale, shift)
#define POOL_SRC(TT) { if (srcfmt == 0) POOL_GO(TT, 0); else if (srcfmt == 1) POOL_GO(TT, 1); else POOL_GO(TT, 2); }
  if (dtype == SFM_DT_F16) POOL_SRC(F16) else POOL_SRC(BF16)
#undef POOL_SRC
#undef POOL_GO
  return SFM_OK;
}

// sfm_pool_time_affine: out = scale[b, c] * avg(src) + shift[b, c].  Pooling the RAW output of a GroupNorm'd layer with
// the layer's per-(utterance, channel) scale / shift gives the pooled normalised latents without ever writing the
// full-rate normalised tensor (the real / imag latent heads of the PerceptionAgent have no activation after the norm).
extern "C" int sfm_pool_time_affine(const float* src, const float* scale, const float* shift, void* dst16, float* dst32,
                                    int B, int Tin, int Tout, int C, long long ld_src, long long ld_dst, int dtype,
                                    void* stream) {
  return pool_time_go(src, 0, scale, shift, dst16, dst32, B, Tin, Tout, C, ld_src, ld_dst, dtype, stream);
}
// the same on a 16-bit source (the raw latent heads written in the operands' format: half the bytes of the GEMM's output and
// of this pass; the 16-bit rounding of a raw value is below the rounding of the pooled operand it ends up in)
extern "C" int sfm_pool_time_affine16(const void* src16, int src_dtype, const float* scale, const float* shift, void* dst16,
                                      float* dst32, int B, int Tin, int Tout, int C, long long ld_src, long long ld_dst, int dtype,
                                      void* stream) {
  if (src_dtype != SFM_DT_F16 && src_dtype != SFM_DT_BF16) return SFM_ERR_ARG;
  return pool_time_go(src16, src_dtype == SFM_DT_F16 ? 1 : 2, scale, shift, dst16, dst32, B, Tin, Tout, C, ld_src, ld_dst, dtype,
                      stream);
}

extern "C" int sfm_pool_time(const float* src, void* dst16, float* dst32, int B, int Tin, int Tout, int C,
                             long long ld_src, long long ld_dst, int dtype, void* stream) {
  return sfm_pool_time_affine(src, nullptr, nullptr, dst16, dst32, B, Tin, Tout, C, ld_src, ld_dst, dtype, stream);
}

// adjoint of pool_time: dsrc[b, t, c] = sum over the windows i that contain t of dout[b, i, c] / |window i|
// A thread owns VEC neighbouring channels (16-byte accesses when VEC = 4) and walks 16 consecutive source rows; the window
// arithmetic is done once per row by every lane alike (scalar), the stream is the [B, Tin, C] fp32 write.
template <int VEC>
__global__ __launch_bounds__(256) void pool_time_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dsrc, int Tin,
                                                            int Tout, int C, long long ld_dout, long long ld_dsrc) {
  constexpr int ROWS = 16;
  const int b = blockIdx.z;
  const int nv = C / VEC;                                   // channel vectors per row
  const int per = 256 / nv > 0 ? 256 / nv : 1;              // rows handled side by side by one block (C <= 256 * VEC)
  const int cv = threadIdx.x % nv, tr = threadIdx.x / nv;
  const int v = blockIdx.x * 256 + threadIdx.x;             // (C > 256 * VEC: blockIdx.x walks the channel vectors)
  const int c = (nv >= 256 ? v : cv) * VEC;
  if (c >= C || (nv < 256 && tr >= per)) return;
  const int t0 = (blockIdx.y * (nv >= 256 ? 1 : per) + (nv >= 256 ? 0 : tr)) * ROWS;
  for (int t = t0; t < min(Tin, t0 + ROWS); ++t) {
    long long lo = ((long long)t * Tout) / Tin;
    long long hi = (((long long)(t + 1)) * Tout + Tin - 1) / Tin - 1;
    if (hi > Tout - 1) hi = Tout - 1;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (long long i = lo; i <= hi; ++i) {
      const long long s_ = (i * Tin) / Tout, e_ = ((i + 1) * Tin + Tout - 1) / Tout;
      const float w = 1.0f / (float)(e_ - s_);
      const float* src = dout + ((long long)b * Tout + i) * ld_dout + c;
      if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        acc[0] += q.x * w; acc[1] += q.y * w; acc[2] += q.z * w; acc[3] += q.w * w;
      } else {
        acc[0] += src[0] * w;
      }
    }
    float* dst = dsrc + ((long long)b * Tin + t) * ld_dsrc + c;
    if (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else dst[0] = acc[0];
  }
}

extern "C" int sfm_pool_time_bwd(const float* dout, float* dsrc, int B, int Tin, int Tout, int C, long long ld_dout,
                                 long long ld_dsrc, void* stream) {
  if (!dout || !dsrc) return SFM_ERR_ARG;
  if (B <= 0 || Tin <= 0 || Tout <= 0 || C <= 0 || B > 65535) return SFM_ERR_SHAPE;
  const bool vec = (C % 4 == 0) && (ld_dout % 4 == 0) && (ld_dsrc % 4 == 0) && (((uintptr_t)dout | (uintptr_t)dsrc) % 16 == 0);
  const int nv = vec ? C / 4 : C;
  const int per = nv >= 256 ? 1 : 256 / nv;
  const long long row_blocks = ((long long)Tin + 16LL * per - 1) / (16LL * per);
  if (row_blocks > 65535) return SFM_ERR_SHAPE;
  dim3 grid(nv >= 256 ? (nv + 255) / 256 : 1, (unsigned)row_blocks, B), block(256);
  if (vec) SFM_LAUNCH((pool_time_bwd_kernel<4>), grid, block, 0, (hipStream_t)stream, dout, dsrc, Tin, Tout, C, ld_dout, ld_dsrc);
  else SFM_LAUNCH((pool_time_bwd_kernel<1>), grid, block, 0, (hipStream_t)stream, dout, dsrc, Tin, Tout, C, ld_dout, ld_dsrc);
  return SFM_OK;
}

// mean over time (glue G2: the episodic-memory key is the mean latent of the utterance): src fp32 [B, T, ld] cols [0, C) ->
// dst fp32 [B, C].  Two deterministic passes: 64-row partial sums, then their sum in a fixed order (a single workgroup per
// (utterance, 256 channels) walking all T rows is latency-bound: 3.4 ms at T 6001).
__global__ __launch_bounds__(256) void mean_time_partial_kernel(const float* __restrict__ src, float* __restrict__ part, int T, int C,
                                                                long long ld, int nchunk) {
  const int b = blockIdx.z, k = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int t0 = k * 64, t1 = min(T, t0 + 64);
  float acc = 0.f;
  for (int t = t0; t < t1; ++t) acc += src[((long long)b * T + t) * ld + c];
  part[((long long)b * nchunk + k) * C + c] = acc;
}

__global__ __launch_bounds__(256) void mean_time_final_kernel(const float* __restrict__ part, float* __restrict__ dst, float scale,
                                                              int C, int nchunk) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float acc = 0.f;
  for (int k = 0; k < nchunk; ++k) acc += part[((long long)b * nchunk + k) * C + c];
  dst[(long long)b * C + c] = acc * scale;
}

extern "C" long long sfm_mean_time_scratch_floats(int B, int T, int C) { return (long long)B * ((T + 63) / 64) * C; }

extern "C" int sfm_mean_time(const float* src, float* dst, float* scratch, int B, int T, int C, long long ld_src, void* stream) {
  if (!src || !dst || !scratch) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || C <= 0 || B > 65535 || ld_src < C) return SFM_ERR_SHAPE;
  const int nchunk = (T + 63) / 64;
  SFM_LAUNCH(mean_time_partial_kernel, dim3((C + 255) / 256, nchunk, B), dim3(256), 0, (hipStream_t)stream, src, scratch, T, C, ld_src,
             nchunk);
  SFM_LAUNCH(mean_time_final_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, scratch, dst, 1.0f / (float)T, C,
             nchunk);
  return SFM_OK;
}

// sum over time with the same two passes (training: gradient of a per-utterance bias broadcast over the frames, glue G3)
extern "C" int sfm_sum_time(const float* src, float* dst, float* scratch, int B, int T, int C, long long ld_src, void* stream) {
  if (!src || !dst || !scratch) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || C <= 0 || B > 65535 || ld_src < C) return SFM_ERR_SHAPE;
  const int nchunk = (T + 63) / 64;
  SFM_LAUNCH(mean_time_partial_kernel, dim3((C + 255) / 256, nchunk, B), dim3(256), 0, (hipStream_t)stream, src, scratch, T, C, ld_src,
             nchunk);
  SFM_LAUNCH(mean_time_final_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, scratch, dst, 1.0f, C, nchunk);
  return SFM_OK;
}

// log1p-magnitude normalisation of the noisy STFT (agents/msa.py:134-137) written as
// 16-bit into the fusion operand: cols [0,F) real, [F,2F) imag, [2F, 2F+zpad) zero.
// One wave per row, a lane per frequency bin: the magnitude and its log1p are computed ONCE per bin for both parts (the per-output-element
// form of rounds 1-3 - 2 square roots, 2 log1pf and a 64-bit division per bin - was bound by those ~200 instructions per bin:
// 1 TB/s).  sqrt / rcp / log by the hardware instructions (1 ulp); below mag = 2^-5, where log(1 + mag) loses its leading
// digits, the series 1 - mag/2 + mag^2/3 - mag^3/4 (next term < 2e-7); the result is rounded to 16 bits.
template <class T>
__global__ __launch_bounds__(256) void stft_lognorm_pack_rows_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                                     u16* __restrict__ dst, long long M, int F, int zpad,
                                                                     long long ld_dst) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* rr = re + m * F;
  const float* ii = im + m * F;
  u16* d = dst + m * ld_dst;
  for (int f = lane; f < F; f += 64) {
    const float r = rr[f], i = ii[f];
    const float mag = __builtin_amdgcn_sqrtf(r * r + i * i + 1e-8f);
    const float nf = mag < 0.03125f ? 1.0f - mag * (0.5f - mag * (0.33333333f - mag * 0.25f))
                                    : __logf(1.0f + mag) * __builtin_amdgcn_rcpf(mag);
    d[f] = T::from_f32(r * nf);
    d[F + f] = T::from_f32(i * nf);
  }
  for (int c = 2 * F + lane; c < 2 * F + zpad; c += 64) d[c] = 0;
}

extern "C" int sfm_stft_lognorm_pack(const float* re, const float* im, void* dst, long long M, int F, int zpad,
                                     long long ld_dst, int dtype, void* stream) {
  if (!re || !im || !dst) return SFM_ERR_ARG;
  if (M <= 0 || F <= 0 || zpad < 0) return SFM_ERR_SHAPE;
  if (M > 4LL * 2147483647LL) return SFM_ERR_SHAPE;
  const unsigned nbr = (unsigned)((M + 3) / 4);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((stft_lognorm_pack_rows_kernel<F16>), dim3(nbr), dim3(256), 0, (hipStream_t)stream, re, im, (u16*)dst, M, F, zpad, ld_dst);
  else
    SFM_LAUNCH((stft_lognorm_pack_rows_kernel<BF16>), dim3(nbr), dim3(256), 0, (hipStream_t)stream, re, im, (u16*)dst, M, F, zpad, ld_dst);
  return SFM_OK;
}

// adjoint of the normalisation above (training with a noisy STFT that carries a gradient): g[m, 0:F) / g[m, F:2F) are the
// gradients of the normalised real / imaginary parts (fp32, leading dimension ld_g);  with n(mag) = log1p(mag) / mag,
//   d re = g_r n + (g_r re + g_i im) n'(mag) re / mag,   n'(mag) = (1 / (1 + mag) - n) / mag      (and the same for im)
__global__ __launch_bounds__(256) void stft_lognorm_bwd_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                               const float* __restrict__ g, float* __restrict__ dre,
                                                               float* __restrict__ dim_, long long M, int F, long long ld_g) {
  const long long total = M * F;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long m = e / F;
    const int f = (int)(e - m * F);
    const float r = re[e], i = im[e];
    const float gr = g[m * ld_g + f], gi = g[m * ld_g + F + f];
    const float mag = sqrtf(r * r + i * i + 1e-8f);
    const float nf = log1pf(mag) / mag;
    const float c = (gr * r + gi * i) * (1.0f / (1.0f + mag) - nf) / (mag * mag);
    dre[e] = gr * nf + c * r;
    dim_[e] = gi * nf + c * i;
  }
}

extern "C" int sfm_stft_lognorm_bwd(const float* re, const float* im, const float* g, float* dre, float* dim_, long long M, int F,
                                    long long ld_g, void* stream) {
  if (!re || !im || !g || !dre || !dim_) return SFM_ERR_ARG;
  if (M <= 0 || F <= 0 || ld_g < 2 * F) return SFM_ERR_SHAPE;
  long long nb = (M * F + 255) / 256;
  if (nb > 16384) nb = 16384;
  SFM_LAUNCH(stft_lognorm_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, re, im, g, dre, dim_, M, F, ld_g);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// Bounded polar mask + complex application (agents/msa.py:166-172,
// models/conformer.py:243-244, training/conformer_pipeline.py:287-296).
//   mag = sigmoid(lm (+ bias[b])) ; ph = tanh(lp) * phase_scale
//   mask = mag * (cos ph, sin ph) ; enh = mask (x) noisy   (optional)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void polar_mask_kernel(const float* __restrict__ lm, const float* __restrict__ lp,
                                                         const float* __restrict__ mag_bias, const float* __restrict__ nr,
                                                         const float* __restrict__ ni, float* mr, float* mi, float* er,
                                                         float* ei, float* mmag, long long rows_per_batch, int F,
                                                         long long total, float phase_scale, long long ld_l,
                                                         long long ld_enh) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    long long m = e / F;
    int f = (int)(e - m * F);
    float a = lm[m * ld_l + f];
    if (mag_bias) a += mag_bias[(m / rows_per_batch) * F + f];
    float mg = 1.0f / (1.0f + expf(-a));
    float ph = tanhf(lp[m * ld_l + f]) * phase_scale;
    float c = cosf(ph), s = sinf(ph);
    float xr = mg * c, xi = mg * s;
    if (mr) mr[e] = xr;
    if (mi) mi[e] = xi;
    if (mmag) mmag[e] = mg;
    if (er) {
      float r = nr[e], i = ni[e];
      er[m * ld_enh + f] = xr * r - xi * i;
      ei[m * ld_enh + f] = xr * i + xi * r;
    }
  }
}

extern "C" int sfm_polar_mask(const float* lm, const float* lp, const float* mag_bias, const float* nr, const float* ni,
                              float* mr, float* mi, float* er, float* ei, float* mmag, int B, long long rows_per_batch,
                              int F, float phase_scale, long long ld_logits, long long ld_enh, void* stream) {
  if (!lm || !lp) return SFM_ERR_ARG;
  if (er && (!ei || !nr || !ni)) return SFM_ERR_ARG;
  long long total = (long long)B * rows_per_batch * F;
  if (total <= 0) return SFM_ERR_SHAPE;
  long long nb = (total + 255) / 256;
  if (nb > 16384) nb = 16384;
  SFM_LAUNCH(polar_mask_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, lm, lp, mag_bias, nr, ni,
                     mr, mi, er, ei, mmag, rows_per_batch, F, total, phase_scale, ld_logits, ld_enh);
  return SFM_OK;
}

// complex multiply (ComplexConformer.apply_mask, models/conformer.py:243-244)
__global__ __launch_bounds__(256) void complex_mul_kernel(const float* __restrict__ sr, const float* __restrict__ si,
                                                          const float* __restrict__ mr, const float* __restrict__ mi,
                                                          float* er, float* ei, long long total) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    float a = sr[e], b = si[e], c = mr[e], d = mi[e];
    er[e] = c * a - d * b;
    ei[e] = c * b + d * a;
  }
}

extern "C" int sfm_complex_mul(const float* sr, const float* si, const float* mr, const float* mi, float* er, float* ei,
                               long long total, void* stream) {
  if (!sr || !si || !mr || !mi || !er || !ei) return SFM_ERR_ARG;
  if (total <= 0) return SFM_ERR_SHAPE;
  long long nb = (total + 255) / 256;
  if (nb > 16384) nb = 16384;
  SFM_LAUNCH(complex_mul_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, sr, si, mr, mi, er, ei,
                     total);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// iSTFT overlap-add (gather form, no atomics) of windowed irfft frames
// frames [B, T, win] (already x window, restricted to the window support):
//   out[b, s] = sum_t frames[b, t, p - t*hop - woff] / sum_t w^2[p - t*hop - woff],
//   p = s + n_fft/2, woff = (n_fft - win)/2   (torch.istft, center=True)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win2,
                                                        float* __restrict__ out, int Tn, int L, int n_fft, int hop,
                                                        int win, long long ld_frames) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= L) return;
  const int p = s + n_fft / 2 - (n_fft - win) / 2;     // position relative to window support start
  int t = p / hop;
  if (t > Tn - 1) t = Tn - 1;
  float acc = 0.f, env = 0.f;
  for (; t >= 0; --t) {
    int n = p - t * hop;
    if (n >= win) break;
    if (n >= 0) {
      acc += frames[((long long)b * Tn + t) * ld_frames + n];
      env += win2[n];
    }
  }
  out[(long long)b * L + s] = (env > 1e-11f) ? acc / env : 0.f;
}

// Packed form: frames [sum_T, ld_frames] and out [sum_L] hold B utterances back to back (frames of utterance u = rows
// [frame_off[u], frame_off[u + 1]), its samples = out[samp_off[u] .. samp_off[u + 1])); each sample finds its utterance by a
// binary search and sums that utterance's frames only, in the dense kernel's order.
__global__ __launch_bounds__(256) void istft_ola_varlen_kernel(const float* __restrict__ frames, const float* __restrict__ win2,
                                                               float* __restrict__ out, const int* __restrict__ frame_off,
                                                               const int* __restrict__ samp_off, int nutt, int sum_L, int n_fft,
                                                               int hop, int win, long long ld_frames) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= sum_L) return;
  const int u = sfm_seg_find(samp_off, nutt, g);
  const int s = g - samp_off[u];
  const int row0 = frame_off[u], Tn = frame_off[u + 1] - row0;
  const int p = s + n_fft / 2 - (n_fft - win) / 2;     // position relative to window support start
  int t = p / hop;
  if (t > Tn - 1) t = Tn - 1;
  float acc = 0.f, env = 0.f;
  for (; t >= 0; --t) {
    int n = p - t * hop;
    if (n >= win) break;
    if (n >= 0) {
      acc += frames[((long long)row0 + t) * ld_frames + n];
      env += win2[n];
    }
  }
  out[g] = (env > 1e-11f) ? acc / env : 0.f;
}

extern "C" int sfm_istft_ola_varlen(const float* frames, const float* win2, float* out, const int* frame_off, const int* samp_off,
                                    int B, int sum_L, int n_fft, int hop, int win, long long ld_frames, void* stream) {
  if (!frames || !win2 || !out || !frame_off || !samp_off) return SFM_ERR_ARG;
  if (B <= 0 || sum_L <= 0 || hop <= 0 || win <= 0 || win > n_fft || ld_frames < win) return SFM_ERR_SHAPE;
  SFM_LAUNCH(istft_ola_varlen_kernel, dim3((sum_L + 255) / 256), dim3(256), 0, (hipStream_t)stream, frames, win2, out, frame_off,
             samp_off, B, sum_L, n_fft, hop, win, ld_frames);
  return SFM_OK;
}

extern "C" int sfm_istft_ola(const float* frames, const float* win2, float* out, int B, int T, int L, int n_fft, int hop,
                             int win, long long ld_frames, void* stream) {
  if (!frames || !win2 || !out) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || L <= 0 || hop <= 0 || win <= 0 || win > n_fft) return SFM_ERR_SHAPE;
  SFM_LAUNCH(istft_ola_kernel, dim3((L + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, frames, win2, out,
                     T, L, n_fft, hop, win, ld_frames);
  return SFM_OK;
}

// pack [real | imag] fp32 rows into one [M, ld] fp32 operand (zero tail) for the irfft GEMM
__global__ __launch_bounds__(256) void pack_spec_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                        float* __restrict__ dst, long long M, int F, int ld,
                                                        long long ld_src) {
  long long total = M * ld;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    long long m = e / ld;
    int c = (int)(e - m * ld);
    float v = 0.f;
    if (c < F) v = re[m * ld_src + c];
    else if (c < 2 * F) v = im[m * ld_src + c - F];
    dst[e] = v;
  }
}

extern "C" int sfm_pack_spec(const float* re, const float* im, float* dst, long long M, int F, int ld, long long ld_src,
                             void* stream) {
  if (!re || !im || !dst) return SFM_ERR_ARG;
  if (M <= 0 || F <= 0 || ld < 2 * F) return SFM_ERR_SHAPE;
  long long nb = (M * ld + 255) / 256;
  if (nb > 16384) nb = 16384;
  SFM_LAUNCH(pack_spec_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, re, im, dst, M, F, ld,
                     ld_src);
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// SincConv1d filter synthesis (agents/perception.py:88-112), one block per
// channel.  Writes filt[c][k] (row-major, for inspection) and Wt[k][c] (k-major,
// zero padded to [Kpad][Npad]: the framed-GEMM operand).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sinc_filters_kernel(const float* __restrict__ low_hz, const float* __restrict__ band_hz,
                                                           const float* __restrict__ window, const float* __restrict__ n_,
                                                           float* filt, float* Wt, int C, int K, int Npad,
                                                           float sample_rate, float min_low, float min_band) {
  __shared__ float red[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int half = (K - 1) / 2;
  float low = min_low + fabsf(low_hz[c]);
  float high = fminf(low + min_band + fabsf(band_hz[c]), sample_rate / 2.0f);
  float fl = low / sample_rate, fh = high / sample_rate;
  float total = 0.f;
  float vals[2] = {0.f, 0.f};
  for (int i = 0; i < 2; ++i) {
    int k = tid + 256 * i;
    float v = 0.f;
    if (k < K) {
      if (k == half) v = 2.0f * (fh - fl);
      else {
        int kk = (k < half) ? k : (K - 1 - k);
        float n = n_[kk];
        v = (sinf(fh * n) - sinf(fl * n)) / (n / 2.0f + 1e-8f);
      }
      v *= window[k];
    }
    vals[i] = v;
    total += fabsf(v);
  }
  total = wave_sum(total);
  if ((tid & 63) == 0) red[tid >> 6] = total;
  __syncthreads();
  float norm = red[0] + red[1] + red[2] + red[3] + 1e-8f;
  for (int i = 0; i < 2; ++i) {
    int k = tid + 256 * i;
    if (k < K) {
      float v = vals[i] / norm;
      if (filt) filt[(long long)c * K + k] = v;
      if (Wt) Wt[(long long)k * Npad + c] = v;
    }
  }
}

extern "C" int sfm_sinc_filters(const float* low_hz, const float* band_hz, const float* window, const float* n_,
                                float* filt, float* Wt, int C, int K, int Npad, float sample_rate, float min_low_hz,
                                float min_band_hz, void* stream) {
  if (!low_hz || !band_hz || !window || !n_ || (!filt && !Wt)) return SFM_ERR_ARG;
  if (C <= 0 || K <= 0 || K > 512 || (K & 1) == 0 || (Wt && Npad < C)) return SFM_ERR_SHAPE;
  SFM_LAUNCH(sinc_filters_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, low_hz, band_hz, window, n_, filt,
                     Wt, C, K, Npad, sample_rate, min_low_hz, min_band_hz);
  return SFM_OK;
}
