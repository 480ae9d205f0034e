// The reference's two remaining intelligibility measures (evaluation/csii.py, evaluation/ncm.py) on the device.
//
// CSII: compute_csii calls _magnitude_squared_coherence on the WHOLE signal for every amplitude region, so
//   the score is clip(sum_f w_f msc_f, 0, 1) of one coherence estimate over all frames.  The spectra come from the packed fp32
//   framed DFT (sfm_framed_gemm_f32_varlen with the Hamming rfft(., 256) operand); csii_frames_kernel sums |X|^2, |Y|^2 and
//   X conj(Y) per (utterance, bin) over the utterance's frames in frame order, in fp64.
//
// NCM: per gammatone channel the normalised covariance of the two Hilbert envelopes.  scipy.signal.hilbert(x).imag is the circular
//   convolution y[n] = sum_m h[(n - m) mod L] x[m] with h = imag(ifft(H)) (H = 1 at 0 and the Nyquist bin, 2 below it): no FFT,
//   the same shape of work as gammatone.hip with the roles of table and signal swapped.  Exact fp32 MFMA (v_mfma_f32_32x32x2_f32):
//   rows of a tile are 32 consecutive output samples, columns 128 channel-signals of one utterance (clean channel c in column c,
//   enhanced channel c in column 64 + c: the two land in the same lane of tiles j and j + 2), a k-step is 2 input samples.
//   A = h[(n - m) mod L] is one LDS word per lane from a staged window of the table (consecutive addresses over the lanes; the
//   table is stored twice back to back, index n - m + L, so the wrap costs no modulo; for an even L every even lag of h is exactly
//   0 and the problem splits into two of half the size, see the kernel), B = x[m][col] one LDS word per lane from a
//   staged [SFM_HE_KSTEP][128] tile.  A staged k-step of SFM_HE_KSTEP = 64 samples is one accumulation segment: the chain restarts with it and
//   the segments are added in order.  The analytic signal is never stored: the epilogue forms env = sqrt(x^2 + y^2) in fp64 and
//   either writes it (sfm_hilbert_env) or five fp64 sums per (utterance, channel, output tile) that ncm_finish_kernel folds in
//   tile order.  No atomics; nothing depends on the pack: an utterance gets the bits it gets alone.
#include "sfm_common.h"

#define HE_WAVES 8
static_assert(SFM_HE_ROWS == HE_WAVES * 32, "output samples per workgroup (the output tile): one 32-row MFMA tile per wave");
static_assert(SFM_HE_KSTEP == 64, "input samples per staged k-step = one accumulation segment: one per lane (xs[lane])");
#define HE_COLS 128                   // columns of the x tile (2 x 64 channel-signals)
#define HE_XLD 129                    // row stride of the x tile in LDS (floats): conflict-free by sample and by column
#define HE_WIN (SFM_HE_ROWS + SFM_HE_KSTEP)      // floats kept for the table window (SFM_HE_ROWS + SFM_HE_KSTEP - 1 used)
#define HE_XPT (SFM_HE_KSTEP * HE_COLS / (HE_WAVES * 64))   // x words staged per thread and k-step (16)
#define HE_LDS_BYTES (HE_WAVES * 2 * 64 * 5 * 8)     // the epilogue's fp64 exchange; >= (HE_WIN + SFM_HE_KSTEP * HE_XLD) * 4

// ENV = 1: x [R, L], workgroup (tile, group of 128 rows), env [R, L]; tiles and table of an even L as below.
// ENV = 0: x = X [2, B, C, L] (clean, enhanced; 0 from lengths[b] on), workgroup i = tiles[i] = (utterance, output tile),
//          tab_off[b] = the utterance's table (2 lengths[b] floats) inside tab, partial [n_tiles, C, 5] fp64.
// Table of an odd length: h twice; of an even length: g_0 twice, then g_1 twice (2 x Lb / 2 floats each).
template <int ENV>
__global__ __launch_bounds__(HE_WAVES * 64) void hilbert_kernel(const float* __restrict__ x, const float* __restrict__ tab,
                                                                const int* __restrict__ tab_off, const int* __restrict__ lengths,
                                                                const int* __restrict__ tiles, float* __restrict__ env,
                                                                double* __restrict__ partial, int B, int C, int L, int R) {
  __shared__ __attribute__((aligned(16))) unsigned char dsm[HE_LDS_BYTES];
  float* hs = reinterpret_cast<float*>(dsm);                   // [HE_WIN]: hs[i] = hh[n0 - m0 - (SFM_HE_KSTEP - 1) + Lc + i], 0 outside [0, 2 Lc)
  float* xs = hs + HE_WIN;                                     // [SFM_HE_KSTEP][HE_XLD]: xs[k][col] = sample m0 + k of the column's convolution, 0 from Lc on
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hl = lane >> 5;
  int b, t, Lb;
  if (ENV) {
    b = blockIdx.y; t = blockIdx.x; Lb = L;
  } else {
    b = tiles[2 * blockIdx.x]; t = tiles[2 * blockIdx.x + 1];
    if (b < 0 || b >= B || t < 0) return;
    Lb = lengths[b];
    Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  }
  // an even length splits: h has no even lag, so the outputs 2 i + p are the circular convolution of length Lb / 2 of the inputs
  // 2 j + 1 - p with g_p[d] = h[(2 d + 2 p - 1) mod Lb]; tiles [0, ntp) are p = 0, [ntp, 2 ntp) p = 1, the table holds g_0 twice, g_1 twice
  const bool even = (Lb & 1) == 0;
  const int Lc = even ? Lb >> 1 : Lb, xst = even ? 2 : 1;       // samples of the convolution, stride of its samples in x
  const int ntp = (Lc + SFM_HE_ROWS - 1) / SFM_HE_ROWS;
  const int par = (even && ntp > 0) ? t / ntp : 0;
  if (even) t -= par * ntp;
  const int xin = even ? 1 - par : 0, xout = even ? par : 0;    // first input / output sample in x
  const int n0 = t * SFM_HE_ROWS;
  if (n0 >= Lc || par > 1) {                                   // a tile behind the utterance (tables that disagree with lengths)
    if (!ENV)
      for (int i = tid; i < C * 5; i += HE_WAVES * 64) partial[(long long)blockIdx.x * C * 5 + i] = 0.0;
    return;
  }
  const float* hh = tab + (ENV ? 0 : tab_off[b]) + (long long)par * Lb;
  // this thread's staging columns: wave + 8 i; its sample of a k-step: lane
  const float* xcol[HE_XPT];
#pragma unroll
  for (int i = 0; i < HE_XPT; ++i) {
    const int col = wave + HE_WAVES * i;
    if (ENV) {
      const long long row = (long long)b * HE_COLS + col;
      xcol[i] = row < R ? x + row * L : nullptr;
    } else {
      const int s = col >> 6, c = col & 63;
      xcol[i] = c < C ? x + (((long long)s * B + b) * C + c) * L : nullptr;
    }
  }
  float xr[HE_XPT], hr = 0.f;
  auto fetch = [&](int m0) {                                   // global -> registers, one k-step ahead of the MFMAs
#pragma unroll
    for (int i = 0; i < HE_XPT; ++i) xr[i] = (xcol[i] && m0 + lane < Lc) ? xcol[i][xst * (m0 + lane) + xin] : 0.f;
    const int idx = n0 - m0 - (SFM_HE_KSTEP - 1) + Lc + tid;
    hr = (tid < SFM_HE_ROWS + SFM_HE_KSTEP - 1 && idx >= 0 && idx < 2 * Lc) ? hh[idx] : 0.f;
  };

  f32x16 acc[4], tot[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = tot[j][r] = 0.f;
  const bool active = n0 + wave * 32 < Lc;                     // this wave's 32 rows hold a sample of the utterance
  const float* ap = hs + wave * 32 + l31 + (SFM_HE_KSTEP - 1) - hl;
  const float* bp = xs + hl * HE_XLD + l31;
  fetch(0);
  for (int m0 = 0; m0 < Lc; m0 += SFM_HE_KSTEP) {
    __syncthreads();                                           // the previous k-step's operand reads are done
#pragma unroll
    for (int i = 0; i < HE_XPT; ++i) xs[lane * HE_XLD + wave + HE_WAVES * i] = xr[i];
    if (tid < HE_WIN) hs[tid] = hr;
    __syncthreads();
    if (m0 + SFM_HE_KSTEP < Lc) fetch(m0 + SFM_HE_KSTEP);
    if (active) {
#pragma unroll 8
      for (int q = 0; q < SFM_HE_KSTEP / 2; ++q) {
        const float a = ap[-2 * q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[2 * q * HE_XLD + j * 32], acc[j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          tot[j][r] += acc[j][r];
          acc[j][r] = 0.f;
        }
    }
  }

  if (ENV) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long row = (long long)b * HE_COLS + j * 32 + l31;
      if (!active || row >= R) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = n0 + wave * 32 + mfma_row(r, lane), n = xst * i + xout;
        if (i >= Lc) continue;
        const double xv = (double)x[row * L + n], yv = (double)tot[j][r];
        env[row * L + n] = (float)sqrt(xv * xv + yv * yv);
      }
    }
    return;
  }

  // five sums per (channel, half-wave) over the lane's 16 rows in register order, then over the 16 (wave, half) parts in order
  double* red = reinterpret_cast<double*>(dsm);                // [HE_WAVES][2][64][5]
  __syncthreads();                                             // the operand images are dead
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = j * 32 + l31;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (active && c < C) {
      const float* xc = x + ((long long)b * C + c) * L;
      const float* xe = x + (((long long)B + b) * C + c) * L;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = n0 + wave * 32 + mfma_row(r, lane), n = xst * i + xout;
        if (i >= Lc) continue;
        const double cx = (double)xc[n], cy = (double)tot[j][r], ex = (double)xe[n], ey = (double)tot[j + 2][r];
        const double ec = sqrt(cx * cx + cy * cy), ee = sqrt(ex * ex + ey * ey);
        s[0] += ec;
        s[1] += ee;
        s[2] = fma(ec, ec, s[2]);
        s[3] = fma(ee, ee, s[3]);
        s[4] = fma(ec, ee, s[4]);
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) red[(((wave * 2 + hl) * 64) + c) * 5 + q] = s[q];
  }
  __syncthreads();
  for (int item = tid; item < C * 5; item += HE_WAVES * 64) {
    double s = 0.0;
    for (int p = 0; p < HE_WAVES * 2; ++p) s += red[p * 64 * 5 + item];   // item = c * 5 + q
    partial[(long long)blockIdx.x * C * 5 + item] = s;
  }
}

// partial [n_tiles, C, 5] = {sum ec, sum ee, sum ec^2, sum ee^2, sum ec ee} -> ncc [B, C], score [B] (ncm.py:35-55, :106-124).
// One workgroup per utterance, thread c folds channel c's tiles [tile_off[b], tile_off[b + 1]) in tile order; an utterance that
// owns no tile (fewer than 64 samples) scores 0.
__global__ __launch_bounds__(64) void ncm_finish_kernel(const double* __restrict__ partial, const int* __restrict__ tile_off,
                                                        const int* __restrict__ lengths, const double* __restrict__ w,
                                                        double* __restrict__ ncc, double* __restrict__ score, int C) {
  __shared__ double term[64];
  const int b = blockIdx.x, c = threadIdx.x;
  const int t0 = tile_off[b], t1 = tile_off[b + 1];
  double val = 0.0;
  if (c < C && t1 > t0) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = t0; t < t1; ++t)
#pragma unroll
      for (int q = 0; q < 5; ++q) s[q] += partial[((long long)t * C + c) * 5 + q];
    const double n = (double)lengths[b];
    const double mc = s[0] / n, me = s[1] / n;
    const double vx = fmax(s[2] / n - mc * mc, 0.0), vy = fmax(s[3] / n - me * me, 0.0), cov = s[4] / n - mc * me;
    const double den = sqrt(vx * vy);
    val = den < 1e-10 ? 0.0 : fmin(fmax(cov / den, -1.0), 1.0);
  }
  if (c < C) ncc[(long long)b * C + c] = val;
  term[c] = c < C ? w[c] * fmax(val, 0.0) : 0.0;
  __syncthreads();
  if (c == 0) {
    double s = 0.0;
    for (int i = 0; i < C; ++i) s += term[i];
    score[b] = fmin(fmax(s, 0.0), 1.0);
  }
}

// spectra rows [sum_frames, 129] of the clean (cr, ci) and the enhanced (er, ei) signal; utterance b owns rows
// [frame_off[b], frame_off[b + 1]).  One workgroup per utterance, thread f owns bin f: frames in frame order, bins in bin order.
__global__ __launch_bounds__(192) void csii_frames_kernel(const float* __restrict__ cr, const float* __restrict__ ci,
                                                          const float* __restrict__ er, const float* __restrict__ ei,
                                                          const int* __restrict__ frame_off, const double* __restrict__ w,
                                                          double* __restrict__ score, double* __restrict__ msc) {
  __shared__ double term[SFM_CSII_BINS];
  const int b = blockIdx.x, f = threadIdx.x;
  const int f0 = frame_off[b], f1 = frame_off[b + 1];
  if (f < SFM_CSII_BINS) {
    double pxx = 0.0, pyy = 0.0, pr = 0.0, pi = 0.0;
#pragma unroll 4
    for (int n = f0; n < f1; ++n) {
      const long long off = (long long)n * SFM_CSII_BINS + f;
      const double a0 = cr[off], a1 = ci[off], b0 = er[off], b1 = ei[off];
      pxx += a0 * a0 + a1 * a1;
      pyy += b0 * b0 + b1 * b1;
      pr += a0 * b0 + a1 * b1;                                 // X conj(Y)
      pi += a1 * b0 - a0 * b1;
    }
    double m = 0.0;
    if (f1 > f0) {
      const double cnt = (double)(f1 - f0);
      pxx /= cnt; pyy /= cnt; pr /= cnt; pi /= cnt;
      m = fmin(fmax((pr * pr + pi * pi) / (pxx * pyy + 1e-10), 0.0), 1.0);
    }
    if (msc) msc[(long long)b * SFM_CSII_BINS + f] = m;
    term[f] = w[f] * m;
  }
  __syncthreads();
  if (f == 0) {
    double s = 0.0;
    for (int i = 0; i < SFM_CSII_BINS; ++i) s += term[i];
    score[b] = f1 > f0 ? fmin(fmax(s, 0.0), 1.0) : 0.0;
  }
}

extern "C" int sfm_csii_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, const int* frame_off,
                                      const double* weights, double* score, double* msc, int B, int sum_frames, int F,
                                      void* stream) {
  if (!cr || !ci || !er || !ei || !frame_off || !weights || !score) return SFM_ERR_ARG;
  if (B <= 0 || sum_frames < 0 || F != SFM_CSII_BINS) return SFM_ERR_SHAPE;
  SFM_LAUNCH(csii_frames_kernel, dim3(B), dim3(192), 0, (hipStream_t)stream, cr, ci, er, ei, frame_off, weights, score, msc);
  return SFM_OK;
}

extern "C" int sfm_hilbert_env(const float* x, const float* table, float* env, int R, int L, void* stream) {
  if (!x || !table || !env) return SFM_ERR_ARG;
  if (R < 1 || L < 1 || L > (1 << 30) - 1 || (R + HE_COLS - 1) / HE_COLS > 65535) return SFM_ERR_SHAPE;
  const int Lc = (L & 1) ? L : L / 2;                          // an even L: two convolutions of half the length
  const dim3 grid(((L & 1) ? 1 : 2) * ((Lc + SFM_HE_ROWS - 1) / SFM_HE_ROWS), (R + HE_COLS - 1) / HE_COLS);
  SFM_LAUNCH((hilbert_kernel<1>), grid, dim3(HE_WAVES * 64), 0, (hipStream_t)stream, x, table, (const int*)nullptr,
             (const int*)nullptr, (const int*)nullptr, env, (double*)nullptr, 1, 0, L, R);
  return SFM_OK;
}

extern "C" int sfm_hilbert_env_moments(const float* X, const float* tables, const int* tab_off, const int* lengths,
                                       const int* tiles, double* partial, int B, int C, int L, int n_tiles, void* stream) {
  if (!X || !tables || !tab_off || !lengths || !tiles || !partial) return SFM_ERR_ARG;
  if (B < 1 || C < 1 || C > 64 || 2 * C > HE_COLS || L < 1 || L > (1 << 30) - 1 || n_tiles < 0) return SFM_ERR_SHAPE;
  if (n_tiles == 0) return SFM_OK;
  SFM_LAUNCH((hilbert_kernel<0>), dim3(n_tiles), dim3(HE_WAVES * 64), 0, (hipStream_t)stream, X, tables, tab_off, lengths, tiles,
             (float*)nullptr, partial, B, C, L, 0);
  return SFM_OK;
}

extern "C" int sfm_ncm_finish(const double* partial, const int* tile_off, const int* lengths, const double* weights, double* ncc,
                              double* score, int B, int C, void* stream) {
  if (!partial || !tile_off || !lengths || !weights || !ncc || !score) return SFM_ERR_ARG;
  if (B < 1 || C < 1 || C > 64) return SFM_ERR_SHAPE;
  SFM_LAUNCH(ncm_finish_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, partial, tile_off, lengths, weights, ncc, score, C);
  return SFM_OK;
}
