// The DNN front end of signal_processing/features.py: per frame [AMS 15 | RASTA-PLP 13 | MFCC 13 | GFCC 13], and its context.
//
// cepstral_kernel: one wave per row, [power or energy -> filterbank (M <= 64) -> log / cube root -> DCT rows], written at a column
//   offset of the [.., ld_out] matrix.  The row's input is either a spectrum row of the exact-fp32 framed GEMM ([re | im], F bins:
//   power re^2 + im^2, or its square root) or two neighbouring hop-block energies of sfm_gammatone_tf (sum y^2, divided by the
//   window: the filtered signal is never stored).  The filterbank [M][F] sits in LDS (lane m walks row m: stride F words, F odd
//   for both banks, so the 32 lanes of a group touch 32 banks; the power row is a broadcast), the DCT rows transposed [M][16]
//   (lane k walks column k).  Sums are fmaf chains in bin order; the logarithm, the cube root and the DCT run in fp64.
// rasta_kernel: one wave per utterance, lane = bark band: lfilter([.2, .1, 0, -.1, -.2], [1, -.98]) along the utterance's own
//   frames from a zero state (direct form II transposed, as scipy), exp, equal loudness, cube root, the mean over its T_b frames in
//   frame order, the DCT of the means, all fp64; the coefficient vector goes to every row of the utterance.  Latency-bound.
// context_kernel: row n = rows clamp(n - ctx .. n + ctx, 0, T_b - 1) side by side, optionally nan / inf -> 0, (f - mean) / std,
//   clip to +-clip, in that order; rows from T_b on are 0.  8-byte accesses (the row widths 54 and 594 are even, not multiples of 4).
// rows_mean_kernel: the per-utterance mean over frames of the stand-alone extractors, fp64 in frame order.
// No atomics anywhere: the same bits from run to run, and for an utterance alone or in a batch.
#include "sfm_common.h"

#define FE_WAVES 4
#define FE_ROWS 64                    // rows per workgroup (16 per wave): amortises the filterbank's load into LDS
#define FE_PLD 260                    // per-wave power row (floats)
static_assert(SFM_FE_MAX_FILTERS <= 64 && SFM_FE_MAX_COEFFS <= 64, "one lane per filter, one lane per DCT row");
static_assert(SFM_FE_MAX_BINS <= FE_PLD, "a row's bins fit the per-wave power row");

__device__ __forceinline__ int fe_frames(const int* lengths, int b, int L, int frame, int hop) {
  int Lb = lengths ? lengths[b] : L;
  Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  return Lb >= frame ? (Lb - frame) / hop + 1 : 0;
}

// in_mode 0: in = spectrum rows [B T][ld_in], re at [0, F), im at [im_off, im_off + F): p = re^2 + im^2; 1: the same, p = sqrt;
//         2: in = partial [B, P, F, 5]: p[c] = (partial[b, bmul n + badd, c, 0] + partial[b, bmul n + badd + 1, c, 0]) / window.
// fb [M][F] or NULL (M == F: the row itself).  compress 0 none, 1 log(v + 1e-10), 2 sign(v) |v|^(1/3).
// dct [NC][M] or NULL (NC == 0: the M values themselves).  out[(b T + n) ld_out + col_off + j], rows n < T_b only.
__global__ __launch_bounds__(FE_WAVES * 64) void cepstral_kernel(const float* __restrict__ in, const float* __restrict__ fb,
                                                                 const float* __restrict__ dct, const int* __restrict__ lengths,
                                                                 float* __restrict__ out, int B, int T, int L, int frame, int hop,
                                                                 int in_mode, long long ld_in, int im_off, int F, int M, int NC,
                                                                 int compress, int P, int bmul, int badd, float window,
                                                                 long long ld_out, int col_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  double* vs = reinterpret_cast<double*>(dsm);                 // [FE_WAVES][SFM_FE_MAX_FILTERS]
  float* ps = reinterpret_cast<float*>(vs + FE_WAVES * SFM_FE_MAX_FILTERS);   // [FE_WAVES][FE_PLD]
  float* dts = ps + FE_WAVES * FE_PLD;                         // [M][SFM_FE_MAX_COEFFS]: dct transposed
  float* fbs = dts + SFM_FE_MAX_FILTERS * SFM_FE_MAX_COEFFS;                       // [M][F]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (fb)
    for (int i = tid; i < M * F; i += FE_WAVES * 64) fbs[i] = fb[i];
  if (dct)
    for (int i = tid; i < NC * M; i += FE_WAVES * 64) dts[(i % M) * SFM_FE_MAX_COEFFS + i / M] = dct[i];
  __syncthreads();
  const long long nrows = (long long)B * T;
  float* pw = ps + wave * FE_PLD;
  double* vw = vs + wave * SFM_FE_MAX_FILTERS;
  for (int it = 0; it < FE_ROWS / FE_WAVES; ++it) {            // uniform over the workgroup: every wave meets every barrier
    const long long row = (long long)blockIdx.x * FE_ROWS + it * FE_WAVES + wave;
    const int b = row < nrows ? (int)(row / T) : 0, n = (int)(row - (long long)b * T);
    const bool live = row < nrows && n < fe_frames(lengths, b, L, frame, hop);
    if (live) {
      if (in_mode == SFM_CEP_BLOCKS) {
        if (lane < F) {
          const float* p0 = in + (((long long)b * P + (long long)bmul * n + badd) * F + lane) * 5;
          pw[lane] = (float)(((double)p0[0] + (double)p0[(long long)F * 5]) / (double)window);
        }
      } else {
        const float* re = in + row * ld_in;
        for (int f = lane; f < F; f += 64) {
          const float a = re[f], c = re[im_off + f];
          const float p = fmaf(a, a, c * c);
          pw[f] = in_mode == SFM_CEP_MAGNITUDE ? sqrtf(p) : p;
        }
      }
    }
    __syncthreads();
    if (live && lane < M) {
      float e;
      if (fb) {
        const float* fr = fbs + lane * F;
        e = 0.f;
        for (int f = 0; f < F; ++f) e = fmaf(fr[f], pw[f], e);
      } else {
        e = pw[lane];
      }
      double v = (double)e;
      if (compress == SFM_CEP_LOG) v = log(v + 1e-10);
      else if (compress == SFM_CEP_CBRT) v = copysign(cbrt(fabs(v)), v);
      vw[lane] = v;
      if (NC == 0) out[row * ld_out + col_off + lane] = (float)v;
    }
    __syncthreads();
    if (live && lane < NC) {
      double c = 0.0;
      for (int m = 0; m < M; ++m) c = fma((double)dts[m * SFM_FE_MAX_COEFFS + lane], vw[m], c);
      out[row * ld_out + col_off + lane] = (float)c;
    }
  }
}

// logb [B, T, M] fp32 (log bark energies), eql [M], dct [NC][M] fp64 -> out[(b T + n) ld_out + col_off + k], n < T_b.  grid B, block 64.
__global__ __launch_bounds__(64) void rasta_kernel(const float* __restrict__ logb, const double* __restrict__ eql,
                                                   const double* __restrict__ dct, const int* __restrict__ lengths,
                                                   float* __restrict__ out, int T, int L, int frame, int hop, int M, int NC,
                                                   long long ld_out, int col_off) {
  __shared__ double mean[SFM_FE_MAX_FILTERS];
  __shared__ float coef[SFM_FE_MAX_COEFFS];
  const int lane = threadIdx.x, b = blockIdx.x;
  int Tb = fe_frames(lengths, b, L, frame, hop);
  Tb = Tb > T ? T : Tb;
  if (Tb <= 0) return;
  if (lane < M) {
    const float* xp = logb + (long long)b * T * M + lane;
    const double q = eql[lane];
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0, sum = 0.0;
    for (int n = 0; n < Tb; ++n) {
      const double x = (double)xp[(long long)n * M];
      const double y = 0.2 * x + z0;                           // direct form II transposed, a = [1, -0.98]
      z0 = 0.1 * x + z1 + 0.98 * y;
      z1 = 0.0 * x + z2;
      z2 = -0.1 * x + z3;
      z3 = -0.2 * x;
      sum += cbrt(exp(y) * q);
    }
    mean[lane] = sum / (double)Tb;
  }
  __syncthreads();
  if (lane < NC) {
    double c = 0.0;
    for (int m = 0; m < M; ++m) c = fma(dct[lane * M + m], mean[m], c);
    coef[lane] = (float)c;
  }
  __syncthreads();
  float* ob = out + (long long)b * T * ld_out + col_off;
  for (int i = lane; i < Tb * NC; i += 64) {
    const int n = i / NC, k = i - n * NC;
    ob[(long long)n * ld_out + k] = coef[k];
  }
}

// feat [B, T, D] -> out [B, T, (2 ctx + 1) D]; D even.  mean / std [(2 ctx + 1) D] or NULL.  A workgroup takes 4 rows.
__global__ __launch_bounds__(256) void context_kernel(const float* __restrict__ feat, const float* __restrict__ mean,
                                                      const float* __restrict__ stdv, const int* __restrict__ lengths,
                                                      float* __restrict__ out, int B, int T, int L, int frame, int hop, int D, int ctx,
                                                      float clip) {
  const int W2 = (2 * ctx + 1) * D / 2, D2 = D / 2;            // in float2 units
  const long long nrows = (long long)B * T;
  for (int r = 0; r < 4; ++r) {
    const long long row = (long long)blockIdx.x * 4 + r;
    if (row >= nrows) return;
    const int b = (int)(row / T), n = (int)(row - (long long)b * T);
    int Tb = fe_frames(lengths, b, L, frame, hop);
    Tb = Tb > T ? T : Tb;
    float2* op = reinterpret_cast<float2*>(out + row * 2 * W2);
    const float2* fp = reinterpret_cast<const float2*>(feat + (long long)b * T * D);
    for (int i = threadIdx.x; i < W2; i += 256) {
      float2 v = make_float2(0.f, 0.f);
      if (n < Tb) {
        const int j = i / D2, f = i - j * D2;
        int s = n - ctx + j;
        s = s < 0 ? 0 : (s > Tb - 1 ? Tb - 1 : s);
        v = fp[(long long)s * D2 + f];
        if (mean) {
          const float2 mu = reinterpret_cast<const float2*>(mean)[i], sd = reinterpret_cast<const float2*>(stdv)[i];
          float e[2] = {v.x, v.y};
          const float m2[2] = {mu.x, mu.y}, s2[2] = {sd.x, sd.y};
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            double x = isfinite(e[q]) ? (double)e[q] : 0.0;
            x = (x - (double)m2[q]) / (double)s2[q];
            x = x < -(double)clip ? -(double)clip : (x > (double)clip ? (double)clip : x);   // np.clip: a nan stays a nan
            e[q] = (float)x;
          }
          v = make_float2(e[0], e[1]);
        }
      }
      op[i] = v;
    }
  }
}

// in [B, T, ld_in] at col_off, N columns -> out [B, N] = sum over n < T_b of the column / den, den = T_b (den_mode 0) or
// max(T_b, 1) given by the caller as `den` (den_mode 1: extract_ams divides by its num_segs); 0 when T_b = 0.  grid B, block 64.
__global__ __launch_bounds__(64) void rows_mean_kernel(const float* __restrict__ in, const int* __restrict__ lengths,
                                                       float* __restrict__ out, int T, int L, int frame, int hop, long long ld_in,
                                                       int col_off, int N, int den) {
  const int b = blockIdx.x;
  int Tb = fe_frames(lengths, b, L, frame, hop);
  Tb = Tb > T ? T : Tb;
  for (int j = threadIdx.x; j < N; j += 64) {
    const float* p = in + (long long)b * T * ld_in + col_off + j;
    double s = 0.0;
    for (int n = 0; n < Tb; ++n) s += (double)p[(long long)n * ld_in];
    const int d = den > 0 ? den : Tb;
    out[(long long)b * N + j] = d > 0 ? (float)(s / (double)d) : 0.f;
  }
}

static int fe_lds_bytes(int M, int F, bool fb) {
  return FE_WAVES * SFM_FE_MAX_FILTERS * 8 + (FE_WAVES * FE_PLD + SFM_FE_MAX_FILTERS * SFM_FE_MAX_COEFFS + (fb ? M * F : 0)) * 4;
}

static bool fe_framing_ok(int B, int T, int L, int frame, int hop) {
  return B > 0 && T > 0 && frame > 0 && hop > 0 && L >= frame && T <= (L - frame) / hop + 1 && (long long)B * T < (1LL << 31);
}

extern "C" int sfm_cepstral(const float* in, const float* fb, const float* dct, const int* lengths, float* out, int B, int T, int L,
                            int frame, int hop, int in_mode, long long ld_in, int im_off, int F, int M, int NC, int compress, int P,
                            int bmul, int badd, float window, long long ld_out, int col_off, void* stream) {
  if (!in || !out || (NC > 0 && !dct)) return SFM_ERR_ARG;
  if (!fe_framing_ok(B, T, L, frame, hop) || in_mode < SFM_CEP_POWER || in_mode > SFM_CEP_BLOCKS || compress < SFM_CEP_NONE ||
      compress > SFM_CEP_CBRT || F < 1 || F > SFM_FE_MAX_BINS || M < 1 || M > SFM_FE_MAX_FILTERS || NC < 0 ||
      NC > SFM_FE_MAX_COEFFS || (!fb && M != F) || col_off < 0 || col_off + (NC ? NC : M) > ld_out)
    return SFM_ERR_SHAPE;
  if (in_mode == SFM_CEP_BLOCKS) {
    if (F > 64 || bmul < 1 || badd < 0 || !(window > 0.f) || (long long)bmul * (T - 1) + badd + 1 >= P) return SFM_ERR_SHAPE;
  } else if (im_off < F || (long long)im_off + F > ld_in) {
    return SFM_ERR_SHAPE;
  }
  const long long nrows = (long long)B * T;
  SFM_LAUNCH_LDS(cepstral_kernel, dim3((unsigned)((nrows + FE_ROWS - 1) / FE_ROWS)), dim3(FE_WAVES * 64), fe_lds_bytes(M, F, fb != nullptr),
                 (hipStream_t)stream, in, fb, dct, lengths, out, B, T, L, frame, hop, in_mode, ld_in, im_off, F, M, NC, compress, P, bmul,
                 badd, window, ld_out, col_off);
  return SFM_OK;
}

extern "C" int sfm_rasta(const float* logb, const double* eql, const double* dct, const int* lengths, float* out, int B, int T, int L,
                         int frame, int hop, int M, int NC, long long ld_out, int col_off, void* stream) {
  if (!logb || !eql || !dct || !out) return SFM_ERR_ARG;
  if (!fe_framing_ok(B, T, L, frame, hop) || M < 1 || M > SFM_FE_MAX_FILTERS || NC < 1 || NC > SFM_FE_MAX_COEFFS || col_off < 0 ||
      col_off + NC > ld_out)
    return SFM_ERR_SHAPE;
  SFM_LAUNCH(rasta_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, logb, eql, dct, lengths, out, T, L, frame, hop, M, NC, ld_out,
             col_off);
  return SFM_OK;
}

extern "C" int sfm_feature_context(const float* feat, const float* mean, const float* stdv, const int* lengths, float* out, int B,
                                   int T, int L, int frame, int hop, int D, int ctx, float clip, void* stream) {
  if (!feat || !out || (mean == nullptr) != (stdv == nullptr)) return SFM_ERR_ARG;
  if (!fe_framing_ok(B, T, L, frame, hop) || D < 2 || (D & 1) || ctx < 0 || ctx > 64 || !(clip > 0.f)) return SFM_ERR_SHAPE;
  const long long nrows = (long long)B * T;
  SFM_LAUNCH(context_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, feat, mean, stdv, lengths, out, B, T,
             L, frame, hop, D, ctx, clip);
  return SFM_OK;
}

extern "C" int sfm_rows_mean(const float* in, const int* lengths, float* out, int B, int T, int L, int frame, int hop, long long ld_in,
                             int col_off, int N, int den, void* stream) {
  if (!in || !out) return SFM_ERR_ARG;
  if (!fe_framing_ok(B, T, L, frame, hop) || N < 1 || col_off < 0 || col_off + N > ld_in || den < 0) return SFM_ERR_SHAPE;
  SFM_LAUNCH(rows_mean_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, in, lengths, out, T, L, frame, hop, ld_in, col_off, N, den);
  return SFM_OK;
}

// ---- the Dataset's statistics over the context rows, from the packed raw rows (training/pipeline.py:246-256 of the reference) -----
// Column k = j D + c of the context row of packed frame n is raw[clamp(n - ctx + j, lo_n, hi_n - 1), c] (bounds[n] = {lo_n, hi_n}:
// the frame's utterance), nan / inf read as 0: the [N, K] rows are never formed.  Two passes in fp64, because a column's mean can
// lie far above its spread (MFCC c0) and raw moments would cancel: pass 0 sums the values, pass 1 the squares of (value - mean).
// context_moments_partial_kernel: grid (chunks, ceil(K / 256)), a thread owns one column over the chunk's rows -> ws[chunk K + k];
// context_moments_fold_kernel: one workgroup adds the chunks in chunk order: the same bits from run to run.
static_assert(SFM_MOMENTS_MAX_CHUNKS == 1024 && SFM_MOMENTS_CHUNK_ROWS == 256, "ws = (SFM_MOMENTS_MAX_CHUNKS + 1) K doubles");

__global__ __launch_bounds__(256) void context_moments_partial_kernel(const float* __restrict__ raw, const int* __restrict__ bounds,
                                                                      const double* __restrict__ mean_d, double* __restrict__ ws,
                                                                      int N, int D, int ctx, int K, int rows_per_chunk) {
  const int k = blockIdx.y * 256 + threadIdx.x;
  if (k >= K) return;
  const int j = k / D, c = k - j * D;
  const int n0 = blockIdx.x * rows_per_chunk;
  const int n1 = n0 + rows_per_chunk < N ? n0 + rows_per_chunk : N;
  const double mu = mean_d ? mean_d[k] : 0.0;
  double s = 0.0;
  for (int n = n0; n < n1; ++n) {
    const int2 lh = *reinterpret_cast<const int2*>(bounds + 2 * (long long)n);
    const int lo = lh.x < 0 ? 0 : lh.x, hi = lh.y > N ? N : lh.y;
    double x = 0.0;
    if (lo < hi) {
      int r = n - ctx + j;
      r = r < lo ? lo : (r > hi - 1 ? hi - 1 : r);
      const float f = raw[(long long)r * D + c];
      x = isfinite(f) ? (double)f : 0.0;
    }
    const double d = x - mu;
    s += mean_d ? d * d : x;
  }
  ws[(long long)blockIdx.x * K + k] = s;
}

__global__ __launch_bounds__(256) void context_moments_fold_kernel(const double* __restrict__ ws, int chunks, int K, int N, int pass,
                                                                   double* __restrict__ mean_d, float* __restrict__ out) {
  for (int k = threadIdx.x; k < K; k += 256) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += ws[(long long)c * K + k];
    if (pass == 0) {
      mean_d[k] = s / (double)N;
      out[k] = (float)(s / (double)N);
    } else {
      const float sd = (float)sqrt(s / (double)N);
      out[k] = sd < 1e-6f ? 1.0f : sd;                                       // a constant column: no division by zero
    }
  }
}

extern "C" int sfm_context_moments(const float* raw, const int* bounds, float* mean, float* stdv, double* ws, int N, int D, int ctx,
                                   void* stream) {
  if (!raw || !bounds || !mean || !stdv || !ws) return SFM_ERR_ARG;
  if (N <= 0 || D < 1 || ctx < 0 || ctx > 64 || (long long)D * (2 * ctx + 1) > (1 << 20)) return SFM_ERR_SHAPE;
  if ((((uintptr_t)bounds) % 8) != 0) return SFM_ERR_ARG;
  const int K = D * (2 * ctx + 1);
  int chunks = (int)sfm_capped_blocks(N, SFM_MOMENTS_CHUNK_ROWS, SFM_MOMENTS_MAX_CHUNKS);
  const int rows_per_chunk = (N + chunks - 1) / chunks;
  chunks = (N + rows_per_chunk - 1) / rows_per_chunk;
  double* mean_d = ws + (long long)SFM_MOMENTS_MAX_CHUNKS * K;
  const dim3 grid((unsigned)chunks, (unsigned)((K + 255) / 256));
  SFM_LAUNCH(context_moments_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, raw, bounds, (const double*)nullptr, ws, N, D, ctx,
             K, rows_per_chunk);
  SFM_LAUNCH(context_moments_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, chunks, K, N, 0, mean_d, mean);
  SFM_LAUNCH(context_moments_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, raw, bounds, (const double*)mean_d, ws, N, D, ctx,
             K, rows_per_chunk);
  SFM_LAUNCH(context_moments_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, chunks, K, N, 1, mean_d, stdv);
  return SFM_OK;
}
