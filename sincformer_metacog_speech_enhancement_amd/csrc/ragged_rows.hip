// Row passes of the ragged front end: the PerceptionAgent and the CPEA run on the zero-padded batch
// [B, rows of the longest utterance, C] with the valid rows of each utterance in an int32 table.  The kernels with tiles of
// their own (sinc_fir16, conv16p, headpool, the BiLSTM) have ragged forms beside their dense ones; here are the three passes
// that belong to no such kernel:
//   sfm_gn_finalize_varlen  sfm_gn_finalize with the row count and the number of partial slots per utterance,
//   sfm_gn_apply_varlen     GroupNorm affine + GELU on the valid rows, zeros on the others (the input of the k 3 uncertainty conv),
//   sfm_rows_gather32       the hand-over: rows of the padded layout -> packed rows [sum rows_b, width].
#include "sfm_common.h"

// gn_finalize_kernel (pointwise.hip) with P = p_tab[b] slots of utterance b folded - the same slots in the same order as the
// dense kernel folds for that utterance alone - out of a partial buffer whose batch stride is Pmax slots, and
// count = rows_tab[b] * (C / G).
__global__ __launch_bounds__(64) void gn_finalize_varlen_kernel(const float* __restrict__ partial, const float* __restrict__ w,
                                                                const float* __restrict__ bsh, float* scale, float* shift,
                                                                const int* __restrict__ rows_tab, const int* __restrict__ p_tab,
                                                                int Pmax, int G, int C, float eps) {
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int P = min(max(p_tab[b], 1), Pmax);
  const double count = (double)rows_tab[b] * (double)(C / G);
  double s = 0.0, q = 0.0;
  for (int i0 = lane; i0 < P; i0 += 64 * 8) {
    f32x2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = i0 + 64 * k < P ? i0 + 64 * k : P - 1;
      v[k] = *reinterpret_cast<const f32x2*>(partial + (((long long)b * Pmax + i) * G + g) * 2);
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

// partial [B, Pmax, G, 2] (slots from p_tab[b] on: never read), rows_tab / p_tab int32 [B] (device): rows and partial slots of
// utterance b -> scale, shift [B, C].  Utterance b gets the bits of sfm_gn_finalize(B = 1, P = p_tab[b], rows = rows_tab[b]).
extern "C" int sfm_gn_finalize_varlen(const float* partial, const float* w, const float* b, float* scale, float* shift,
                                      const int* rows_tab, const int* p_tab, int B, int Pmax, int G, int C, float eps, void* stream) {
  if (!partial || !w || !b || !scale || !shift || !rows_tab || !p_tab) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || Pmax <= 0 || G <= 0 || C % G != 0) return SFM_ERR_SHAPE;
  SFM_LAUNCH(gn_finalize_varlen_kernel, dim3(G, B), dim3(64), 0, (hipStream_t)stream, partial, w, b, scale, shift, rows_tab, p_tab,
             Pmax, G, C, eps);
  return SFM_OK;
}

// gn_apply_rows_kernel<T, 1, false> (pointwise.hip) on 16-bit rows with a 16-bit result: y = GELU(x * sc[b, c] + sh[b, c]) by the
// same expression on the rows below rows_tab[b]; the rows from rows_tab[b] on are not read and are written as zeros.
template <class T>
__global__ __launch_bounds__(256) void gn_apply_varlen_kernel(const u16* __restrict__ x1, const float* __restrict__ sc1,
                                                              const float* __restrict__ sh1, u16* __restrict__ out,
                                                              const int* __restrict__ rows_tab, int L, int C, int rows_per_block) {
  const long long b = blockIdx.y;
  const int Lb = min(max(rows_tab[b], 0), L);
  const int nv = C >> 3, rl = 256 / nv;
  const int tv = threadIdx.x % nv, tr = threadIdx.x / nv, c0 = tv * 8;
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  float s1[8], h1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s1[i] = sc1[b * C + c0 + i];
    h1[i] = sh1[b * C + c0 + i];
  }
  for (int l = l0 + tr; l < l1; l += rl) {
    const long long e = (b * L + l) * C + c0;
    u32x4 o = {0u, 0u, 0u, 0u};
    if (l < Lb) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(x1 + e);
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = T::to_f32((u16)(a[i] & 0xffffu));
        v[2 * i + 1] = T::to_f32((u16)(a[i] >> 16));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float y = fmaf(v[i], s1[i], h1[i]);
        y = (fabsf(y) > 3.75f) ? gelu_erf(y) : y * normal_cdf_poly(y);
        v[i] = y;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = pack2<T>(v[2 * i], v[2 * i + 1]);
    }
    *reinterpret_cast<u32x4*>(out + e) = o;
  }
}

// x1, out [B, L, C] 16-bit in `dtype`, sc1 / sh1 [B, C] fp32, rows_tab int32 [B] (device).  C a power of two in [64, 2048].
// out[b, l] = GELU(x1[b, l] * sc1[b] + sh1[b]) for l < rows_tab[b] - the bits of sfm_gn_apply(act = 1) - and 0 from there on.
extern "C" int sfm_gn_apply_varlen(const void* x1, const float* sc1, const float* sh1, void* out, const int* rows_tab, int B, int L,
                                   int C, int dtype, void* stream) {
  if (!x1 || !sc1 || !sh1 || !out || !rows_tab) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || L <= 0 || C < 64 || C > 2048 || (C & (C - 1)) != 0) return SFM_ERR_SHAPE;
  if ((((uintptr_t)x1) | ((uintptr_t)out)) % 16 != 0) return SFM_ERR_SHAPE;
  const int rpb = 8 * (2048 / C) > 256 ? 8 * (2048 / C) : 256;
  dim3 grid((L + rpb - 1) / rpb, B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((gn_apply_varlen_kernel<F16>), grid, block, 0, st, (const u16*)x1, sc1, sh1, (u16*)out, rows_tab, L, C, rpb);
  else SFM_LAUNCH((gn_apply_varlen_kernel<BF16>), grid, block, 0, st, (const u16*)x1, sc1, sh1, (u16*)out, rows_tab, L, C, rpb);
  return SFM_OK;
}

// dst[(dst_off[b] + r) * ld_dst + c] = src[(b * src_rows + r) * ld_src + c] for r < rows_tab[b], c < width, in 32-bit words
__global__ __launch_bounds__(256) void rows_gather32_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                            const int* __restrict__ rows_tab, const int* __restrict__ dst_off,
                                                            int src_rows, int width, long long ld_src, long long ld_dst) {
  const int b = blockIdx.y;
  const long long n = (long long)min(max(rows_tab[b], 0), src_rows) * width;
  const uint32_t* s = src + (long long)b * src_rows * ld_src;
  uint32_t* d = dst + (long long)dst_off[b] * ld_dst;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const long long r = e / width;
    const int c = (int)(e - r * width);
    d[r * ld_dst + c] = s[r * ld_src + c];
  }
}

// The hand-over from the padded layout to the packed one, on 32-bit words (fp32 elements, or pairs of 16-bit ones):
//   src [B, src_rows, ld_src], dst [sum_b rows_tab[b], ld_dst]; rows_tab int32 [B], dst_off int32 [B] (or [B + 1]) = the exclusive
//   prefix sums of rows_tab (device).  Row r < rows_tab[b] of utterance b: its first `width` words go to row dst_off[b] + r of dst.
//   Rows of src from rows_tab[b] on are never read; every word of the `width` columns of dst is written.
extern "C" int sfm_rows_gather32(const void* src, void* dst, const int* rows_tab, const int* dst_off, int B, int src_rows, int width,
                                 long long ld_src, long long ld_dst, void* stream) {
  if (!src || !dst || !rows_tab || !dst_off) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || src_rows <= 0 || width <= 0 || ld_src < width || ld_dst < width) return SFM_ERR_SHAPE;
  if ((((uintptr_t)src) | ((uintptr_t)dst)) % 4 != 0) return SFM_ERR_SHAPE;
  const long long per = ((long long)src_rows * width + 255) / 256;
  dim3 grid((unsigned)(per < 64 ? per : 64), B), block(256);
  SFM_LAUNCH(rows_gather32_kernel, grid, block, 0, (hipStream_t)stream, (const uint32_t*)src, (uint32_t*)dst, rows_tab, dst_off,
             src_rows, width, ld_src, ld_dst);
  return SFM_OK;
}
