// Gammatone T-F analysis (signal_processing/gammatone.py): the causal FIR bank y[c, m] = sum_k h_c[k] x[m - k] on the matrix cores
// and the per-frame quantities of get_tf_magnitudes without an FFT.
//
// For a frame f of w <= N samples and even N, Parseval over the N/2 + 1 rfft bins gives
//   sum_k |S_k|^2 = (N sum f^2 + (sum f)^2 + (sum (-1)^t f)^2) / 2,     S[k] = sum f[t] cos(2 pi k t / N) - i sum f[t] sin(2 pi k t / N)
// so a (channel, frame) needs five sums {f^2, f, (-1)^t f, f cos, f sin}.  With hop = frame / 2 (hop even) they are taken per
// hop-block with the block-local t; frame n = block n + exp(-2 pi i k hop / N) * block n + 1 (sfm_gammatone_tf_finish), and the
// parity sum of a block keeps its sign.  The filtered signal [B, C, L] (256 bytes per sample) then never exists in HBM.
//
// Operands: exact fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, restarted every 64 taps; the segments are added in order).  Rows of a tile are 32 consecutive samples, columns
// 32 channels, a k-step is 2 taps: A = x[m - k] is one LDS word per lane from the staged patch (consecutive addresses over the
// lanes), B = taps[k][c] one global word per lane from the [K][64] table (256 contiguous bytes per half-wave, L2-resident) shared
// by the wave's row tiles.  No Toeplitz operand and no tap image in LDS: K is bounded by the patch only.
// Split 16-bit operands (sinc_fir16's form) were not kept: bf16 hi + lo drops the lo x lo term at 2^-16 of a product, the size of
// 16 e32 of this row, and fp16's range does not hold the taps' tails without a per-channel scale.
//
// A workgroup (4 waves) owns SFM_GT_ROWS = 384 samples (FIR) or the hop-blocks that fit into them (fused), forms y for all channels
// in accumulators (up to 3 row tiles x 2 column tiles per wave), parks the tile in LDS and then either stores it [B, C, L] or
// reduces each hop-block in fp64 in t order.  No atomics; nothing depends on the batch: an utterance gets the bits it gets alone.
#include "sfm_common.h"

#define GT_WAVES 4
#define GT_RT 3                       // row tiles per wave
#define GT_YLD 65                     // row stride of the y tile in LDS (floats): conflict-free by row and by channel
#define GT_KC 4                       // k-steps (of 2 taps) per tap prefetch chunk
#define GT_SEG 8                      // chunks per accumulation segment (64 taps)
static_assert(SFM_GT_ROWS == GT_WAVES * GT_RT * 32, "a workgroup's samples: 32 per row tile of each wave");
static_assert(SFM_GT_COLS == 64, "two 32-column MFMA tiles: C <= 64, padded with zero taps");

template <int NA>
__device__ __forceinline__ void gt_mfma_tiles(const float* __restrict__ taps, const float* xs, float* yt, int K, int wave, int lane) {
  const int l31 = lane & 31, hl = lane >> 5;
  // acc: the MFMA chain of the current segment of GT_SEG chunks (64 taps); tot: the segments, added in tap order.  A chain
  // over all K taps carries sqrt(K) roundings of its partial sums; 64-tap chains plus K / 64 adds carry a third of that at K 800
  f32x16 acc[NA][2], tot[NA][2];
#pragma unroll
  for (int g = 0; g < NA; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[g][j][r] = tot[g][j][r] = 0.f;
  int seg = 0;
  const float* tp = taps + hl * SFM_GT_COLS + l31;
  const float* xp = xs + K + wave * 32 + l31 - hl;            // row tile g of this wave: tile g * GT_WAVES + wave
  // taps of GT_KC k-steps at a time, the next chunk's loads issued before this chunk's MFMAs (K is a multiple of 2 GT_KC)
  float nb[GT_KC][2];
#pragma unroll
  for (int q = 0; q < GT_KC; ++q) {
    nb[q][0] = tp[2 * q * SFM_GT_COLS];
    nb[q][1] = tp[2 * q * SFM_GT_COLS + 32];
  }
  for (int k0 = 0; k0 < K; k0 += 2 * GT_KC) {
    float bq[GT_KC][2];
#pragma unroll
    for (int q = 0; q < GT_KC; ++q) {
      bq[q][0] = nb[q][0];
      bq[q][1] = nb[q][1];
    }
    const int kn = (k0 + 2 * GT_KC < K) ? k0 + 2 * GT_KC : k0;
#pragma unroll
    for (int q = 0; q < GT_KC; ++q) {
      nb[q][0] = tp[(kn + 2 * q) * SFM_GT_COLS];
      nb[q][1] = tp[(kn + 2 * q) * SFM_GT_COLS + 32];
    }
#pragma unroll
    for (int q = 0; q < GT_KC; ++q)
#pragma unroll
      for (int g = 0; g < NA; ++g) {
        const float a = xp[g * (GT_WAVES * 32) - k0 - 2 * q];
        acc[g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq[q][0], acc[g][0], 0, 0, 0);
        acc[g][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bq[q][1], acc[g][1], 0, 0, 0);
      }
    if (++seg == GT_SEG || k0 + 2 * GT_KC >= K) {
      seg = 0;
#pragma unroll
      for (int g = 0; g < NA; ++g)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tot[g][j][r] += acc[g][j][r];
            acc[g][j][r] = 0.f;
          }
    }
  }
#pragma unroll
  for (int g = 0; g < NA; ++g)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        yt[((g * GT_WAVES + wave) * 32 + mfma_row(r, lane)) * GT_YLD + j * 32 + l31] = tot[g][j][r];
}

// sig [B, L]; taps [K][64] (K a multiple of 8); FUSED: tw [2][hop][64] (cos, sin of the block-local t), dst = partial [B, nblocks, C, 5];
// otherwise dst = out [B, C, L].  grid (chunks, B); nb = hop-blocks per workgroup (FUSED).
template <int FUSED>
__global__ __launch_bounds__(GT_WAVES * 64) void gammatone_kernel(const float* __restrict__ sig, const float* __restrict__ taps,
                                                                  const float* __restrict__ tw, const int* __restrict__ lengths,
                                                                  float* __restrict__ dst, int L, int C, int K, int hop, int nblocks,
                                                                  int nb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  float* xs = reinterpret_cast<float*>(dsm);                   // [SFM_GT_ROWS + K]: xs[i] = x[m0 - K + i], 0 outside [0, Lb)
  float* yt = xs + SFM_GT_ROWS + K;                                // [SFM_GT_ROWS][GT_YLD]
  float* tws = yt + SFM_GT_ROWS * GT_YLD;                          // FUSED: [2][hop][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  int Lb = lengths ? lengths[b] : L;
  Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  const int blk0 = blockIdx.x * nb;                            // FUSED: first hop-block of this workgroup
  const int m0 = FUSED ? blk0 * hop : blockIdx.x * SFM_GT_ROWS;
  int nrows;
  if (FUSED) {
    const int nbw = (nblocks - blk0 < nb) ? nblocks - blk0 : nb;
    nrows = nbw * hop;
    if (m0 >= Lb) return;                                      // blocks behind the utterance feed no frame below T_b
  } else {
    nrows = (L - m0 < SFM_GT_ROWS) ? L - m0 : SFM_GT_ROWS;
  }
  const float* xb = sig + (long long)b * L;
  for (int i = tid; i < SFM_GT_ROWS + K; i += GT_WAVES * 64) {
    const int s = m0 - K + i;
    xs[i] = (s >= 0 && s < Lb) ? xb[s] : 0.f;
  }
  if (FUSED)
    for (int i = tid; i < 2 * hop * SFM_GT_COLS; i += GT_WAVES * 64) tws[i] = tw[i];
  __syncthreads();

  const int ntile = (nrows + 31) >> 5;                         // <= GT_WAVES * GT_RT
  const int na = (ntile - wave + GT_WAVES - 1) / GT_WAVES;     // this wave's tiles: wave, wave + 4, wave + 8
  if (na >= 3) gt_mfma_tiles<3>(taps, xs, yt, K, wave, lane);
  else if (na == 2) gt_mfma_tiles<2>(taps, xs, yt, K, wave, lane);
  else if (na == 1) gt_mfma_tiles<1>(taps, xs, yt, K, wave, lane);
  __syncthreads();

  if (!FUSED) {
    for (int c = wave; c < C; c += GT_WAVES) {
      float* op = dst + ((long long)b * C + c) * L + m0;
      for (int r = lane; r < nrows; r += 64) op[r] = (m0 + r < Lb) ? yt[r * GT_YLD + c] : 0.f;
    }
    return;
  }
  const int nbw = nrows / hop;
  for (int item = tid; item < nbw * C; item += GT_WAVES * 64) {
    const int j = item / C, c = item - j * C;
    const float* yp = yt + (j * hop) * GT_YLD + c;
    double s2 = 0.0, s1 = 0.0, sp = 0.0, sc = 0.0, ss = 0.0;
    for (int t = 0; t < hop; ++t) {                            // fixed order: t ascending
      const double y = (double)yp[t * GT_YLD];
      s2 = fma(y, y, s2);
      s1 += y;
      sp += (t & 1) ? -y : y;
      sc = fma(y, (double)tws[t * SFM_GT_COLS + c], sc);
      ss = fma(y, (double)tws[(hop + t) * SFM_GT_COLS + c], ss);
    }
    float* pp = dst + (((long long)b * nblocks + blk0 + j) * C + c) * 5;
    pp[0] = (float)s2; pp[1] = (float)s1; pp[2] = (float)sp; pp[3] = (float)sc; pp[4] = (float)ss;
  }
}

// y [B, C, L] -> partial [B, T, C, 5]: the five sums of frame n = y[b, c, n * hop + t], t < w, with the frame-local t.
// tw [2][w][64].  One wave per (b, c, n): lanes stride t, fp64, one butterfly (every lane holds the same total).
__global__ __launch_bounds__(256) void gammatone_moments_kernel(const float* __restrict__ y, const float* __restrict__ tw,
                                                                const int* __restrict__ lengths, float* __restrict__ partial, int L,
                                                                int C, int T, int w, int hop, int frame) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave, c = blockIdx.y, b = blockIdx.z;
  if (n >= T) return;
  int Lb = lengths ? lengths[b] : L;
  Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  if ((long long)n * hop + frame > Lb) return;                 // n >= T_b: never read by the finish
  const float* yp = y + ((long long)b * C + c) * L + (long long)n * hop;
  double s2 = 0.0, s1 = 0.0, sp = 0.0, sc = 0.0, ss = 0.0;
  for (int t = lane; t < w; t += 64) {
    const double v = (double)yp[t];
    s2 = fma(v, v, s2);
    s1 += v;
    sp += (t & 1) ? -v : v;
    sc = fma(v, (double)tw[t * SFM_GT_COLS + c], sc);
    ss = fma(v, (double)tw[(w + t) * SFM_GT_COLS + c], ss);
  }
  s2 = wave_sum_d(s2); s1 = wave_sum_d(s1); sp = wave_sum_d(sp); sc = wave_sum_d(sc); ss = wave_sum_d(ss);
  if (lane == 0) {
    float* pp = partial + (((long long)b * T + n) * C + c) * 5;
    pp[0] = (float)s2; pp[1] = (float)s1; pp[2] = (float)sp; pp[3] = (float)sc; pp[4] = (float)ss;
  }
}

// partial [B, P, C, 5] -> mag, phase (, re, im) [B, C, T].  two: frame n = rows n and n + 1 (hop-blocks), the second rotated by
// rot [2][64] = (cos, sin)(2 pi k hop / N); otherwise row n alone.  Frames from T_b on are 0.  A workgroup takes 32 frames of one
// utterance: it reads the partials channel-fastest and writes the planes frame-fastest through LDS.
__global__ __launch_bounds__(256) void gammatone_finish_kernel(const float* __restrict__ partial, const float* __restrict__ rot,
                                                               const int* __restrict__ lengths, float* __restrict__ mag,
                                                               float* __restrict__ phase, float* __restrict__ re,
                                                               float* __restrict__ im, int C, int T, int P, int two, int L, int frame,
                                                               int hop, int N) {
  __shared__ float res[4][SFM_GT_COLS][33];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * 32;
  int Lb = lengths ? lengths[b] : L;
  Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  const int Tb = Lb >= frame ? (Lb - frame) / hop + 1 : 0;
  for (int item = tid; item < 32 * C; item += 256) {
    const int i = item / C, c = item - i * C, n = n0 + i;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < T && n < Tb) {
      const float* p0 = partial + (((long long)b * P + n) * C + c) * 5;
      double s2 = p0[0], s1 = p0[1], sp = p0[2], sr = p0[3], si = p0[4];
      if (two) {
        const float* p1 = p0 + (long long)C * 5;
        const double rc = rot[c], rs = rot[SFM_GT_COLS + c], c1 = p1[3], d1 = p1[4];
        s2 += (double)p1[0]; s1 += (double)p1[1]; sp += (double)p1[2];
        sr += rc * c1 - rs * d1;
        si += rc * d1 + rs * c1;
      }
      const double vr = sr, vi = 0.0 - si;
      o[0] = (float)(0.5 * ((double)N * s2 + s1 * s1 + sp * sp));
      o[1] = (float)atan2(vi, vr);
      o[2] = (float)vr;
      o[3] = (float)vi;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) res[q][c][i] = o[q];
  }
  __syncthreads();
  float* dstp[4] = {mag, phase, re, im};
  for (int item = tid; item < 32 * C; item += 256) {
    const int c = item >> 5, i = item & 31, n = n0 + i;
    if (n >= T) continue;
    const long long off = ((long long)b * C + c) * T + n;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (dstp[q]) dstp[q][off] = res[q][c][i];
  }
}

static int gt_lds_bytes(int K, int hop) { return ((SFM_GT_ROWS + K) + SFM_GT_ROWS * GT_YLD + 2 * hop * SFM_GT_COLS) * 4; }

static bool gt_bank_ok(int B, int L, int C, int K) {
  return B > 0 && B <= 65535 && L > 0 && C > 0 && C <= SFM_GT_COLS && K >= 2 * GT_KC && K <= SFM_GT_MAX_TAPS && K % (2 * GT_KC) == 0;
}

extern "C" int sfm_gammatone_fir(const float* sig, const float* taps, const int* lengths, float* out, int B, int L, int C, int K,
                                 void* stream) {
  if (!sig || !taps || !out) return SFM_ERR_ARG;
  if (!gt_bank_ok(B, L, C, K)) return SFM_ERR_SHAPE;
  const dim3 grid((L + SFM_GT_ROWS - 1) / SFM_GT_ROWS, B);
  SFM_LAUNCH_LDS((gammatone_kernel<0>), grid, dim3(GT_WAVES * 64), gt_lds_bytes(K, 0), (hipStream_t)stream, sig, taps,
                 (const float*)nullptr, lengths, out, L, C, K, 0, 0, 0);
  return SFM_OK;
}

// sfm_gammatone_tf takes (K, hop) when the workgroup's LDS image fits and at least one hop-block fits its rows
// (exported: the host's router asks this predicate, ops.gammatone_tf_fits)
extern "C" int sfm_gammatone_tf_fits(int K, int hop) {
  return K >= 2 * GT_KC && K <= SFM_GT_MAX_TAPS && K % (2 * GT_KC) == 0 && hop >= 2 && (hop & 1) == 0 && hop <= SFM_GT_ROWS &&
         gt_lds_bytes(K, hop) <= SFM_GT_LDS_MAX;
}

extern "C" int sfm_gammatone_tf(const float* sig, const float* taps, const float* tw, const int* lengths, float* partial, int B,
                                int L, int C, int K, int hop, int nblocks, void* stream) {
  if (!sig || !taps || !tw || !partial) return SFM_ERR_ARG;
  if (!gt_bank_ok(B, L, C, K) || !sfm_gammatone_tf_fits(K, hop) || nblocks < 1 || (long long)nblocks * hop > L)
    return SFM_ERR_SHAPE;
  const int nb = SFM_GT_ROWS / hop;
  const dim3 grid((nblocks + nb - 1) / nb, B);
  SFM_LAUNCH_LDS((gammatone_kernel<1>), grid, dim3(GT_WAVES * 64), gt_lds_bytes(K, hop), (hipStream_t)stream, sig, taps, tw, lengths,
                 partial, L, C, K, hop, nblocks, nb);
  return SFM_OK;
}

extern "C" int sfm_gammatone_moments(const float* y, const float* tw, const int* lengths, float* partial, int B, int L, int C, int T,
                                     int w, int frame, int hop, void* stream) {
  if (!y || !tw || !partial) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || C <= 0 || C > SFM_GT_COLS || L <= 0 || T <= 0 || w <= 0 || w > frame || hop <= 0 ||
      (long long)(T - 1) * hop + frame > L)
    return SFM_ERR_SHAPE;
  SFM_LAUNCH(gammatone_moments_kernel, dim3((T + 3) / 4, C, B), dim3(256), 0, (hipStream_t)stream, y, tw, lengths, partial, L, C, T, w,
             hop, frame);
  return SFM_OK;
}

extern "C" int sfm_gammatone_tf_finish(const float* partial, const float* rot, const int* lengths, float* mag, float* phase, float* re,
                                       float* im, int B, int C, int T, int P, int two, int L, int frame, int hop, int N,
                                       void* stream) {
  if (!partial || !mag || !phase || (two && !rot)) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || C <= 0 || C > SFM_GT_COLS || T <= 0 || frame <= 0 || hop <= 0 || N < 2 || (N & 1) || L < frame ||
      T > (L - frame) / hop + 1 || P < T + (two ? 1 : 0))
    return SFM_ERR_SHAPE;
  SFM_LAUNCH(gammatone_finish_kernel, dim3((T + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, partial, rot, lengths, mag, phase, re,
             im, C, T, P, two, L, frame, hop, N);
  return SFM_OK;
}
