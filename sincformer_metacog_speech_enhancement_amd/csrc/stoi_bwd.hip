// The gradient of STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) with respect to the ENHANCED signal: stoi.hip walked back.
// The kept list and K belong to the clean signal, so they are constants and the gradient is exact.  Three kernels
// (include/sincformer_hip.h states the layouts):
//   stoi_segments_bwd_kernel  one workgroup per 32 band rows of an utterance, the forward's ring of band rows: the backward of each
//                             15 x 30 segment that holds one of its rows in fp64 (clip decisions recomputed from the same stored
//                             rows), a row's cotangent summed over its up to 30 segments in segment order in an LDS ring and
//                             written once when the last of them has passed; the segments that straddle two workgroups' rows are
//                             computed by both, so no sum crosses a workgroup
//   stoi_bands_bwd_kernel     one workgroup per 16 spectral frames: the A tile and Re | Im as stoi_bands_kernel forms them, each bin
//                             scaled by dband / band, the scaled 16 x 432 tile times the transposed DFT operand on
//                             v_mfma_f64_16x16x4_f64, times the window -> dframes rows
//   stoi_fold_bwd_kernel      the overlap-add adjoint as a gather: one thread per 10 kHz sample, at most 2 x 2 terms in a fixed order
// The resampler's adjoint is stoi_resample_kernel itself with up and down exchanged (evaluation/stoi_taal.py designs its operand).
// A norm at the zero vector and a band value of exactly 0 pass nothing back (never inf * 0).  No atomics; every sum is fp64 in a
// fixed order, so an utterance's bits do not depend on what it is packed with.
#include "sfm_common.h"

#define SB_EPS 2.220446049250313e-16        // np.finfo(np.float64).eps
#define SB_NBIN (SFM_STOI_LAST_BIN - SFM_STOI_FIRST_BIN + 1)
#define SB_AS (SFM_STOI_FRAME + 1)          // A-tile row stride (doubles)
#define SB_CS (SFM_STOI_DFT_COLS + 1)       // product-tile row stride (doubles)
#define SB_RING 64                          // ring rows: >= SFM_STOI_SEG_TILE + SFM_STOI_SEG - 1, a power of two
#define SB_CLIP (1.0 + 5.623413251903491)   // 1 + 10^(15/20)

static __constant__ int sb_edges[SFM_STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
static_assert(SFM_STOI_FRAME == 256 && SFM_STOI_HOP * 2 == SFM_STOI_FRAME, "one thread per sample of a frame, half overlap");
static_assert(SFM_STOI_ROW_TILE == 16 && SFM_STOI_FRAME % 64 == 0, "one 16-row MFMA tile per workgroup, 16 column tiles over four waves");
static_assert(SFM_STOI_DFT_COLS % 16 == 0 && SFM_STOI_DFT_COLS >= 2 * SB_NBIN && SFM_STOI_DFT_COLS % 4 == 0, "column tiles, K steps");
static_assert(SB_CS >= SB_AS, "the product tile covers the A tile");
static_assert(SB_RING >= SFM_STOI_SEG_TILE + SFM_STOI_SEG - 1 && (SB_RING & (SB_RING - 1)) == 0, "ring holds one stage");
static_assert(SFM_STOI_BANDS <= 64 && SFM_STOI_SEG <= 64, "one lane per band / per frame of a segment");

// d(v / (|v| + eps)) applied to a cotangent, for a CENTRED v of norm nv: dv_n = dout_n / (nv + eps) - <dout, v> v_n / (nv (nv + eps)^2);
// the factor of the second term, 0 at the zero vector
__device__ __forceinline__ double sb_norm_pull(double dot, double nv) {
  return nv > 0.0 ? dot / (nv * (nv + SB_EPS) * (nv + SB_EPS)) : 0.0;
}

template <bool EXT>
__global__ __launch_bounds__(256) void stoi_segments_bwd_kernel(const float* __restrict__ xb, const float* __restrict__ yb,
                                                                const int* __restrict__ frame_off, const int* __restrict__ kept,
                                                                const double* __restrict__ gscore, float* __restrict__ dyb) {
  __shared__ float ring[2][SB_RING][SFM_STOI_BANDS];
  __shared__ double dacc[SB_RING][SFM_STOI_BANDS];                           // the open rows' sums
  __shared__ double contrib[4][SFM_STOI_SEG][SFM_STOI_BANDS];               // each wave's segment: d segment / d y rows
  __shared__ double rows[EXT ? 4 : 1][2][SFM_STOI_BANDS][SFM_STOI_SEG];     // ESTOI: the row-normalised block of each wave
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = frame_off[u], nrows = frame_off[u + 1] - f0, M = min(kept[u] - 1, nrows);
  // this workgroup OWNS the rows [R0, R1) of the utterance (zeros: up to Rz): it walks every segment that holds one of them, the
  // up to 29 that reach in from below included, and adds to its own rows only - a row's sum is whole and in segment order
  const int R0 = blockIdx.y * SFM_STOI_BWD_ROWS, Rz = min(R0 + SFM_STOI_BWD_ROWS, nrows);
  if (R0 >= nrows) return;
  float* out = dyb + (long long)f0 * SFM_STOI_BANDS;
  if (M < SFM_STOI_SEG || R0 >= M) {
    for (int i = R0 * SFM_STOI_BANDS + tid; i < Rz * SFM_STOI_BANDS; i += 256) out[i] = 0.f;
    return;
  }
  const int R1 = min(Rz, M);
  const int nseg = M - SFM_STOI_SEG + 1, sA = max(R0 - (SFM_STOI_SEG - 1), 0), sB = min(R1 - 1, nseg - 1);      // sA <= sB
  const double gseg = EXT ? gscore[u] / nseg : gscore[u] / ((double)nseg * SFM_STOI_BANDS);
  for (int i = tid; i < SB_RING * SFM_STOI_BANDS; i += 256) (&dacc[0][0])[i] = 0.0;
  for (int i = R1 * SFM_STOI_BANDS + tid; i < Rz * SFM_STOI_BANDS; i += 256) out[i] = 0.f;
  int loaded = sA;
  for (int s0 = sA; s0 <= sB; s0 += SFM_STOI_SEG_TILE) {
    const int cnt = min(SFM_STOI_SEG_TILE, sB + 1 - s0);
    const int need = s0 + cnt - 1 + SFM_STOI_SEG;            // rows [sA, need) serve the segments up to s0 + cnt - 1; need <= M
    for (int i = loaded * SFM_STOI_BANDS + tid; i < need * SFM_STOI_BANDS; i += 256) {
      const int r = i / SFM_STOI_BANDS, b = i - r * SFM_STOI_BANDS;
      ring[0][r & (SB_RING - 1)][b] = xb[(long long)f0 * SFM_STOI_BANDS + i];
      ring[1][r & (SB_RING - 1)][b] = yb[(long long)f0 * SFM_STOI_BANDS + i];
    }
    loaded = need;
    __syncthreads();
    for (int i0 = 0; i0 < cnt; i0 += 4) {
      const bool active = i0 + wave < cnt;
      const int r0 = s0 + i0 + wave;                          // the segment's first row
      if (!EXT) {
        if (active && lane < SFM_STOI_BANDS) {
          double sx2 = 0.0, sy2 = 0.0, sx = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            sx2 += xv * xv;
            sy2 += yv * yv;
            sx += xv;
          }
          const double nx = sqrt(sx2), ny = sqrt(sy2), alpha = nx / (ny + SB_EPS), mx = sx / SFM_STOI_SEG;
          double sy = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            sy += fmin(alpha * yv, xv * SB_CLIP);
          }
          const double my = sy / SFM_STOI_SEG;
          double sxx = 0.0, syy = 0.0, sxy = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            const double dx = xv - mx, dy = fmin(alpha * yv, xv * SB_CLIP) - my;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
          }
          // d = <u, dx> / ((|dx| + eps)(|u| + eps)), u = z - mean z: du_n = c1 dx_n - c2 u_n
          const double nxc = sqrt(sxx), nu = sqrt(syy);
          const double c1 = gseg / ((nxc + SB_EPS) * (nu + SB_EPS)), c2 = gseg / (nxc + SB_EPS) * sb_norm_pull(sxy, nu);
          double sdu = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            sdu += c1 * (xv - mx) - c2 * (fmin(alpha * yv, xv * SB_CLIP) - my);
          }
          const double mdu = sdu / SFM_STOI_SEG;
          double da = 0.0;                                   // the cotangent of alpha: unclipped elements only
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            const double ay = alpha * yv, cx = xv * SB_CLIP;
            if (!(ay > cx)) da += (c1 * (xv - mx) - c2 * (ay - my) - mdu) * yv;
          }
          const double t = ny > 0.0 ? da * nx / (ny * (ny + SB_EPS) * (ny + SB_EPS)) : 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ring[0][(r0 + n) & (SB_RING - 1)][lane], yv = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
            const double ay = alpha * yv, cx = xv * SB_CLIP;
            const double direct = ay > cx ? 0.0 : alpha * (c1 * (xv - mx) - c2 * (ay - my) - mdu);
            contrib[wave][n][lane] = direct - t * yv;
          }
        }
      } else {
        if (active && lane < SFM_STOI_BANDS) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            double s = 0.0;
            for (int n = 0; n < SFM_STOI_SEG; ++n) s += (double)ring[q][(r0 + n) & (SB_RING - 1)][lane];
            const double mean = s / SFM_STOI_SEG;
            double ss = 0.0;
            for (int n = 0; n < SFM_STOI_SEG; ++n) {
              const double d = (double)ring[q][(r0 + n) & (SB_RING - 1)][lane] - mean;
              ss += d * d;
            }
            const double inv = 1.0 / (sqrt(ss) + SB_EPS);
            for (int n = 0; n < SFM_STOI_SEG; ++n)
              rows[wave][q][lane][n] = ((double)ring[q][(r0 + n) & (SB_RING - 1)][lane] - mean) * inv;
          }
        }
        __syncthreads();
        if (active && lane < SFM_STOI_SEG) {                 // the column normalisation back: a lane owns a frame of the segment
          double sx = 0.0, sy = 0.0;
          for (int b = 0; b < SFM_STOI_BANDS; ++b) {
            sx += rows[wave][0][b][lane];
            sy += rows[wave][1][b][lane];
          }
          const double mx = sx / SFM_STOI_BANDS, my = sy / SFM_STOI_BANDS;
          double sxx = 0.0, syy = 0.0, sxy = 0.0;
          for (int b = 0; b < SFM_STOI_BANDS; ++b) {
            const double dx = rows[wave][0][b][lane] - mx, dy = rows[wave][1][b][lane] - my;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
          }
          const double nxc = sqrt(sxx), nyc = sqrt(syy), gs = gseg / SFM_STOI_SEG;
          const double c1 = gs / ((nxc + SB_EPS) * (nyc + SB_EPS)), c2 = gs / (nxc + SB_EPS) * sb_norm_pull(sxy, nyc);
          double sd = 0.0;
          for (int b = 0; b < SFM_STOI_BANDS; ++b) sd += c1 * (rows[wave][0][b][lane] - mx) - c2 * (rows[wave][1][b][lane] - my);
          const double md = sd / SFM_STOI_BANDS;
          for (int b = 0; b < SFM_STOI_BANDS; ++b)           // the clean block's column is this lane's alone: it becomes the cotangent
            rows[wave][0][b][lane] = c1 * (rows[wave][0][b][lane] - mx) - c2 * (rows[wave][1][b][lane] - my) - md;
        }
        __syncthreads();
        if (active && lane < SFM_STOI_BANDS) {               // the row normalisation back: a lane owns a band
          double s = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) s += (double)ring[1][(r0 + n) & (SB_RING - 1)][lane];
          const double mean = s / SFM_STOI_SEG;
          double ss = 0.0, dot = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double d = (double)ring[1][(r0 + n) & (SB_RING - 1)][lane] - mean;
            ss += d * d;
            dot += rows[wave][0][lane][n] * d;
          }
          const double ny = sqrt(ss), c1 = 1.0 / (ny + SB_EPS), c2 = sb_norm_pull(dot, ny);
          // the mean of c1 g_n - c2 d_n over n: the d_n sum to (numerically) nothing, and are summed all the same
          double sd = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n)
            sd += c1 * rows[wave][0][lane][n] - c2 * ((double)ring[1][(r0 + n) & (SB_RING - 1)][lane] - mean);
          const double md = sd / SFM_STOI_SEG;
          for (int n = 0; n < SFM_STOI_SEG; ++n)
            contrib[wave][n][lane] = c1 * rows[wave][0][lane][n] - c2 * ((double)ring[1][(r0 + n) & (SB_RING - 1)][lane] - mean) - md;
        }
      }
      __syncthreads();
      // the up to four segments g0 .. g1 of this step, added to the owned rows they hold in segment order; row r is finished when
      // segment min(r, nseg - 1) <= sB has passed: written once, its slot cleared for row r + SB_RING
      const int g0 = s0 + i0, g1 = min(g0 + 3, s0 + cnt - 1);
      for (int i = tid; i < (g1 + SFM_STOI_SEG - g0) * SFM_STOI_BANDS; i += 256) {
        const int r = g0 + i / SFM_STOI_BANDS, b = i % SFM_STOI_BANDS;
        if (r < R0 || r >= R1) continue;
        double a = dacc[r & (SB_RING - 1)][b];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int s = g0 + w;
          if (s <= g1 && r >= s && r < s + SFM_STOI_SEG) a += contrib[w][r - s][b];
        }
        const bool done = r <= g1 || g1 == sB;
        if (done) out[r * SFM_STOI_BANDS + b] = (float)a;
        dacc[r & (SB_RING - 1)][b] = done ? 0.0 : a;
      }
      __syncthreads();                                      // (uniform: cnt is the workgroup's) contrib[] and rows[] are free again
    }
  }
}

// v_mfma_f64_16x16x4_f64: A lane l -> A[l & 15][l >> 4], B lane l -> B[l >> 4][l & 15]; where the 4 results of a lane sit in the
// 16 x 16 tile is asked of the instruction itself (two products with index operands), as in stoi.hip.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ __launch_bounds__(256) void stoi_bands_bwd_kernel(const float* __restrict__ sig, const float* __restrict__ win,
                                                             const float* __restrict__ dft, const float* __restrict__ dft_t,
                                                             const int* __restrict__ sig_off, const int* __restrict__ frame_off,
                                                             const int* __restrict__ src, const int* __restrict__ kept,
                                                             const int* __restrict__ tiles, const float* __restrict__ dyb,
                                                             float* __restrict__ dframes) {
  __shared__ double tile[SFM_STOI_ROW_TILE * SB_CS];        // the A tile [16][257], then Re | Im [16][433], then the scaled tile
  __shared__ double scale[SFM_STOI_ROW_TILE][SFM_STOI_BANDS];
  __shared__ int stab[SFM_STOI_ROW_TILE + 2];               // src[m0 - 1 .. m0 + 16]
  __shared__ unsigned char band_of[SB_NBIN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = tiles[2 * blockIdx.x], m0 = tiles[2 * blockIdx.x + 1] * SFM_STOI_ROW_TILE;
  const int f0 = frame_off[u], K = min(kept[u], frame_off[u + 1] - f0), M = K - 1;
  if (m0 >= M || M < SFM_STOI_SEG) return;                  // (below one segment the score is a constant: the fold writes zeros)
  const float* x = sig + sig_off[u];
  if (tid < SFM_STOI_ROW_TILE + 2) {
    const int k = m0 - 1 + tid;
    stab[tid] = (k >= 0 && k < K) ? src[f0 + k] : 0;
  }
  if (tid < SB_NBIN) {
    int b = 0;
    while (b < SFM_STOI_BANDS - 1 && tid + SFM_STOI_FIRST_BIN >= sb_edges[b + 1]) ++b;
    band_of[tid] = (unsigned char)b;
  }
  __syncthreads();
  {                                                         // the A tile exactly as stoi_bands_kernel stages it
    const int n = tid, no = tid ^ SFM_STOI_HOP;
    const double wn = (double)win[n], wo = (double)win[no];
    for (int r = 0; r < SFM_STOI_ROW_TILE; ++r) {
      const int m = m0 + r;
      double z = 0.0;
      if (m < M) {
        double v = wn * (double)x[(long long)stab[r + 1] * SFM_STOI_HOP + n];
        if (n >= SFM_STOI_HOP) v += wo * (double)x[(long long)stab[r + 2] * SFM_STOI_HOP + no];
        else if (m >= 1) v += wo * (double)x[(long long)stab[r] * SFM_STOI_HOP + no];
        z = wn * v;
      }
      tile[r * SB_AS + n] = z;
    }
  }
  __syncthreads();
  const double idx = (lane >> 4) == 0 ? (double)(lane & 15) : 0.0, one = (lane >> 4) == 0 ? 1.0 : 0.0;
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  const f64x4 drow = __builtin_amdgcn_mfma_f64_16x16x4f64(idx, one, zero, 0, 0, 0);
  const f64x4 dcol = __builtin_amdgcn_mfma_f64_16x16x4f64(one, idx, zero, 0, 0, 0);
  {
    constexpr int NCT = SFM_STOI_DFT_COLS / 16;             // 27 column tiles: wave w takes w, w + 4, ..
    constexpr int NJ = (NCT + 3) / 4;
    f64x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = zero;
    const double* ap = tile + (lane & 15) * SB_AS + (lane >> 4);
    const float* bp = dft + (long long)(lane >> 4) * SFM_STOI_DFT_COLS + wave * 16 + (lane & 15);
#pragma unroll 2
    for (int ks = 0; ks < SFM_STOI_FRAME / 4; ++ks) {
      const double a = ap[4 * ks];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (wave + 4 * j < NCT) {
          const double bv = (double)bp[(long long)(4 * ks) * SFM_STOI_DFT_COLS + 64 * j];
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[j], 0, 0, 0);
        }
      }
    }
    __syncthreads();                                        // every wave has read its A fragments: the tile is reused
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (wave + 4 * j < NCT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = min(max((int)drow[r], 0), SFM_STOI_ROW_TILE - 1), col = min(max((int)dcol[r], 0), 15);
          tile[row * SB_CS + (wave + 4 * j) * 16 + col] = acc[j][r];
        }
      }
    }
  }
  __syncthreads();
  // band = sqrt(sum |X|^2) in bin order as the forward sums it; dRe = Re dband / band, nothing where the band is exactly 0
  for (int it = tid; it < SFM_STOI_ROW_TILE * SFM_STOI_BANDS; it += 256) {
    const int r = it / SFM_STOI_BANDS, b = it - r * SFM_STOI_BANDS;
    double sc = 0.0;
    if (m0 + r < M) {
      const double* row = tile + r * SB_CS;
      double s = 0.0;
      for (int c = sb_edges[b] - SFM_STOI_FIRST_BIN; c < sb_edges[b + 1] - SFM_STOI_FIRST_BIN; ++c) {
        const double re = row[c], im = row[SB_NBIN + c];
        s += re * re + im * im;
      }
      if (s > 0.0) sc = (double)dyb[(long long)(f0 + m0 + r) * SFM_STOI_BANDS + b] / sqrt(s);
    }
    scale[r][b] = sc;
  }
  __syncthreads();
  for (int it = tid; it < SFM_STOI_ROW_TILE * 2 * SB_NBIN; it += 256) {
    const int r = it / (2 * SB_NBIN), c = it - r * (2 * SB_NBIN);
    const double sc = scale[r][band_of[c < SB_NBIN ? c : c - SB_NBIN]];
    tile[r * SB_CS + c] = sc == 0.0 ? 0.0 : tile[r * SB_CS + c] * sc;
  }
  __syncthreads();
  // (scaled Re | Im) [16, 432] x dft_t [432, 256]: 16 column tiles, wave w takes w, w + 4, w + 8, w + 12 (columns 424 .. 431 of the
  // tile are the zero columns of the first product)
  constexpr int NJ2 = SFM_STOI_FRAME / 64;
  f64x4 acc2[NJ2];
#pragma unroll
  for (int j = 0; j < NJ2; ++j) acc2[j] = zero;
  const double* ap2 = tile + (lane & 15) * SB_CS + (lane >> 4);
  const float* bp2 = dft_t + (long long)(lane >> 4) * SFM_STOI_FRAME + wave * 16 + (lane & 15);
#pragma unroll 2
  for (int ks = 0; ks < SFM_STOI_DFT_COLS / 4; ++ks) {
    const double a = ap2[4 * ks];
#pragma unroll
    for (int j = 0; j < NJ2; ++j) {
      const double bv = (double)bp2[(long long)(4 * ks) * SFM_STOI_FRAME + 64 * j];
      acc2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc2[j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < NJ2; ++j) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(max((int)drow[r], 0), SFM_STOI_ROW_TILE - 1), col = min(max((int)dcol[r], 0), 15);
      const int n = (wave + 4 * j) * 16 + col;
      if (m0 + row < M) dframes[(long long)(f0 + m0 + row) * SFM_STOI_FRAME + n] = (float)((double)win[n] * acc2[j][r]);
    }
  }
}

// position of source frame f in the ascending kept list s[0 .. K), -1 if it was dropped
__device__ __forceinline__ int sb_kept_pos(const int* __restrict__ s, int K, int f) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  return (lo < K && s[lo] == f) ? lo : -1;
}

__global__ __launch_bounds__(256) void stoi_fold_bwd_kernel(const float* __restrict__ dframes, const float* __restrict__ win,
                                                            const int* __restrict__ sig_off, const int* __restrict__ sig_len,
                                                            const int* __restrict__ frame_off, const int* __restrict__ src,
                                                            const int* __restrict__ kept, float* __restrict__ dsig, int pad_to) {
  const int u = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x, len = sig_len[u];
  if (s >= max(len, pad_to)) return;
  float* out = dsig + (long long)sig_off[u] + s;
  const int f0 = frame_off[u], nf = frame_off[u + 1] - f0, K = min(kept[u], nf), M = K - 1;
  if (s >= len || M < SFM_STOI_SEG) {
    *out = 0.f;
    return;
  }
  double acc = 0.0;
#pragma unroll
  for (int side = 0; side < 2; ++side) {                    // source frame s / 128 - 1 (its second half), then s / 128 (its first)
    const int f = s / SFM_STOI_HOP - 1 + side;
    if (f < 0 || f >= nf) continue;
    const int k = sb_kept_pos(src + f0, K, f);
    if (k < 0) continue;
    const int o = s - f * SFM_STOI_HOP, q = k + (o >> 7), lo = o & (SFM_STOI_HOP - 1);
    double t = 0.0;                                         // the rebuilt sample 128 q + lo lies in spectral frames q - 1 and q
    if (q - 1 >= 0 && q - 1 < M) t += (double)dframes[(long long)(f0 + q - 1) * SFM_STOI_FRAME + lo + SFM_STOI_HOP];
    if (q < M) t += (double)dframes[(long long)(f0 + q) * SFM_STOI_FRAME + lo];
    acc += (double)win[o] * t;
  }
  *out = (float)acc;
}

extern "C" int sfm_stoi_segments_bwd(const float* xb, const float* yb, const int* frame_off, const int* kept, const double* gscore,
                                     float* dyb, int B, int max_rows, int extended, void* stream) {
  if (!xb || !yb || !frame_off || !kept || !gscore || !dyb) return SFM_ERR_ARG;
  if (B <= 0 || max_rows < 0 || max_rows > 65535 * SFM_STOI_BWD_ROWS || (extended != 0 && extended != 1)) return SFM_ERR_SHAPE;
  if (max_rows == 0) return SFM_OK;                         // no utterance has a frame: there is no row
  const dim3 grid(B, (max_rows + SFM_STOI_BWD_ROWS - 1) / SFM_STOI_BWD_ROWS);
  if (extended)
    SFM_LAUNCH(stoi_segments_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, xb, yb, frame_off, kept, gscore, dyb);
  else
    SFM_LAUNCH(stoi_segments_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, xb, yb, frame_off, kept, gscore, dyb);
  return SFM_OK;
}

extern "C" int sfm_stoi_bands_bwd(const float* sig, const float* win, const float* dft, const float* dft_t, const int* sig_off,
                                  const int* frame_off, const int* src, const int* kept, const int* tiles, const float* dyb,
                                  float* dframes, int n_tiles, void* stream) {
  if (!sig || !win || !dft || !dft_t || !sig_off || !frame_off || !src || !kept || !dyb || !dframes) return SFM_ERR_ARG;
  if (n_tiles < 0 || n_tiles > 65535 * 1024) return SFM_ERR_SHAPE;
  if (n_tiles == 0) return SFM_OK;                          // no utterance has a spectral frame: an empty table has no address
  if (!tiles) return SFM_ERR_ARG;
  SFM_LAUNCH(stoi_bands_bwd_kernel, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, sig, win, dft, dft_t, sig_off, frame_off, src,
             kept, tiles, dyb, dframes);
  return SFM_OK;
}

extern "C" int sfm_stoi_fold_bwd(const float* dframes, const float* win, const int* sig_off, const int* sig_len, const int* frame_off,
                                 const int* src, const int* kept, float* dsig, int B, int max_len, int pad_to, void* stream) {
  if (!dframes || !win || !sig_off || !sig_len || !frame_off || !src || !kept || !dsig) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || max_len < 0 || pad_to < 0 || pad_to > max_len) return SFM_ERR_SHAPE;
  if (max_len == 0) return SFM_OK;
  SFM_LAUNCH(stoi_fold_bwd_kernel, dim3((max_len + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, dframes, win, sig_off, sig_len,
             frame_off, src, kept, dsig, pad_to);
  return SFM_OK;
}
