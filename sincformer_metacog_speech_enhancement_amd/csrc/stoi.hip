// STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) at 10 kHz: what evaluation/stoi.py:46-50 of the reference computes when
// pystoi is installed.  Four kernels of the measure (include/sincformer_hip.h states the layouts):
//   stoi_resample_kernel  the polyphase FIR to 10 kHz, fp32 operands, fp64 sums
//   stoi_keep_kernel      one workgroup per utterance: frame energies of the clean signal in fp64, their maximum, the keep mask,
//                         an exclusive scan of the mask -> the list of kept source frames and its length K (device data)
//   stoi_bands_kernel     one workgroup per 16 spectral frames of one signal: the frames are rebuilt from three kept source frames
//                         while staged, windowed (fp64), multiplied by the fp32 256 x 424 DFT operand (bins 7 .. 218) on
//                         v_mfma_f64_16x16x4_f64, squared and summed per one-third-octave band -> rows [., 15]; neither the
//                         rebuilt signal nor the spectrum is ever in memory.  (fp32 accumulation of the 256-term rows moves a
//                         score by up to 1e-7, more than the float32-operand evaluation's own error: profiles/README.md round 26)
//   stoi_segments_kernel  one workgroup per utterance: band rows through a ring in LDS (each read once), the 15 x 30 segment
//                         terms in fp64, added in segment order
// and for the OPT-PCIRM search that climbs this measure (masks/opt_pcirm.py, "fitness": "stoi_taal" / "estoi"):
//   stoi_bands_pair_kernel  stoi_bands_kernel for ya and yb at once -> the fp64 planes P | Q | R of the band energy P + 2 x Q + x^2 R
//   pso_fitness_taal_kernel one workgroup per (particle, utterance): the segment kernel's walk with the enhanced rows formed from the
//                           planes at the particle's x; the segment arithmetic itself (sk_score) exists once
// No atomics; every cross-lane sum is a fixed butterfly in fp64, so an utterance's bits do not depend on what it is packed with.
#include "sfm_common.h"

#define SK_EPS 2.220446049250313e-16        // np.finfo(np.float64).eps
#define SK_NBIN (SFM_STOI_LAST_BIN - SFM_STOI_FIRST_BIN + 1)     // 212 bins -> 424 operand columns
#define SK_AS (SFM_STOI_FRAME + 1)          // A-tile row stride (doubles)
#define SK_CS (SFM_STOI_DFT_COLS + 1)       // result-tile row stride (doubles)
#define SK_RING 64                          // ring rows: >= SFM_STOI_SEG_TILE + SFM_STOI_SEG - 1, a power of two

__constant__ int sk_edges[SFM_STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
static_assert(SFM_STOI_FRAME == 256 && SFM_STOI_HOP * 2 == SFM_STOI_FRAME, "one thread per sample of a frame, half overlap");
static_assert(SFM_STOI_ROW_TILE == 16, "one 16-row MFMA tile per workgroup");
static_assert(SFM_STOI_DFT_COLS % 16 == 0 && SFM_STOI_DFT_COLS >= 2 * SK_NBIN, "column tiles of the four waves");
static_assert(SK_CS >= SK_AS, "the product tile covers the A tile");
static_assert(SK_RING >= SFM_STOI_SEG_TILE + SFM_STOI_SEG - 1 && (SK_RING & (SK_RING - 1)) == 0, "ring holds one stage");
static_assert(SFM_STOI_BANDS <= 64 && SFM_STOI_SEG <= 64, "one lane per band / per frame of a segment");

__global__ __launch_bounds__(256) void stoi_keep_kernel(const float* __restrict__ sig, const float* __restrict__ win,
                                                        const int* __restrict__ sig_off, const int* __restrict__ sig_len,
                                                        const int* __restrict__ frame_off, double* __restrict__ energy,
                                                        int* __restrict__ src, int* __restrict__ kept) {
  __shared__ double wmax[4];
  __shared__ int wcnt[4];
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = frame_off[u], len = sig_len[u];
  int n = frame_off[u + 1] - f0;
  const int nmax = len >= SFM_STOI_FRAME ? (len - SFM_STOI_FRAME) / SFM_STOI_HOP + 1 : 0;
  if (n > nmax) n = nmax;                                   // (never more frames than the samples hold, whatever the table says)
  if (n <= 0) {
    if (tid == 0) kept[u] = 0;
    return;
  }
  const float* x = sig + sig_off[u];
  double w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (double)win[lane * 4 + j];
  double emax = -1.0e300;
  for (int f = wave; f < n; f += 4) {
    const float* xf = x + (long long)f * SFM_STOI_HOP + lane * 4;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double p = w[j] * (double)xf[j];
      s += p * p;
    }
    s = wave_sum_d(s);
    const double e = 20.0 * log10(sqrt(s) + SK_EPS);
    if (lane == 0) energy[f0 + f] = e;
    emax = fmax(emax, e);
  }
  if (lane == 0) wmax[wave] = emax;
  __syncthreads();
  const double thr = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])) - 40.0;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int f = c0 + tid;
    const bool keep = f < n && energy[f0 + f] > thr;
    const unsigned long long m = __ballot(keep);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wave) woff += wcnt[i];
      total += wcnt[i];
    }
    if (keep) src[f0 + base + woff + pre] = f;
    base += total;
    __syncthreads();
  }
  if (tid == 0) kept[u] = base;
}

// v_mfma_f64_16x16x4_f64: A lane l -> A[l & 15][l >> 4], B lane l -> B[l >> 4][l & 15]; where the 4 results of a lane sit in the
// 16 x 16 tile is asked of the instruction itself (two products with index operands), not assumed.
typedef __attribute__((ext_vector_type(4))) double f64x4;

__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ sig0, const float* __restrict__ sig1,
                                                         const float* __restrict__ win, const float* __restrict__ dft,
                                                         const int* __restrict__ sig_off, const int* __restrict__ frame_off,
                                                         const int* __restrict__ src, const int* __restrict__ kept,
                                                         const int* __restrict__ tiles, float* __restrict__ bands0,
                                                         float* __restrict__ bands1) {
  __shared__ double tile[SFM_STOI_ROW_TILE * SK_CS];        // the A tile [16][257], then the products [16][433]
  __shared__ int stab[SFM_STOI_ROW_TILE + 2];               // src[m0 - 1 .. m0 + 16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = tiles[2 * blockIdx.x], m0 = tiles[2 * blockIdx.x + 1] * SFM_STOI_ROW_TILE;
  const int f0 = frame_off[u], K = kept[u], M = K - 1;      // M spectral frames: the last kept frame starts none
  if (m0 >= M) return;
  const float* x = (blockIdx.y ? sig1 : sig0) + sig_off[u];
  float* out = blockIdx.y ? bands1 : bands0;
  if (tid < SFM_STOI_ROW_TILE + 2) {
    const int k = m0 - 1 + tid;
    stab[tid] = (k >= 0 && k < K) ? src[f0 + k] : 0;
  }
  __syncthreads();
  {
    const int n = tid, no = tid ^ SFM_STOI_HOP;
    const double wn = (double)win[n], wo = (double)win[no];
    for (int r = 0; r < SFM_STOI_ROW_TILE; ++r) {
      const int m = m0 + r;
      double z = 0.0;
      if (m < M) {
        double v = wn * (double)x[(long long)stab[r + 1] * SFM_STOI_HOP + n];
        if (n >= SFM_STOI_HOP) v += wo * (double)x[(long long)stab[r + 2] * SFM_STOI_HOP + no];      // head of kept frame m + 1
        else if (m >= 1) v += wo * (double)x[(long long)stab[r] * SFM_STOI_HOP + no];               // tail of kept frame m - 1
        z = wn * v;
      }
      tile[r * SK_AS + n] = z;
    }
  }
  __syncthreads();
  constexpr int NCT = SFM_STOI_DFT_COLS / 16;               // 27 column tiles: wave w takes w, w + 4, .. (7, 7, 7, 6)
  constexpr int NJ = (NCT + 3) / 4;
  f64x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const double* ap = tile + (lane & 15) * SK_AS + (lane >> 4);
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
  // rows and columns of this lane's four results: D = (i in column k = 0) x (ones in row k = 0) gives i, the transpose gives j
  const double idx = (lane >> 4) == 0 ? (double)(lane & 15) : 0.0, one = (lane >> 4) == 0 ? 1.0 : 0.0;
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  const f64x4 drow = __builtin_amdgcn_mfma_f64_16x16x4f64(idx, one, zero, 0, 0, 0);
  const f64x4 dcol = __builtin_amdgcn_mfma_f64_16x16x4f64(one, idx, zero, 0, 0, 0);
  __syncthreads();                                          // every wave has read its A fragments: the tile is reused
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (wave + 4 * j < NCT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = min(max((int)drow[r], 0), SFM_STOI_ROW_TILE - 1), col = min(max((int)dcol[r], 0), 15);
        tile[row * SK_CS + (wave + 4 * j) * 16 + col] = acc[j][r];
      }
    }
  }
  __syncthreads();
  for (int it = tid; it < SFM_STOI_ROW_TILE * SFM_STOI_BANDS; it += 256) {
    const int r = it / SFM_STOI_BANDS, b = it - r * SFM_STOI_BANDS;
    if (m0 + r >= M) continue;
    const double* row = tile + r * SK_CS;
    double s = 0.0;
    for (int c = sk_edges[b] - SFM_STOI_FIRST_BIN; c < sk_edges[b + 1] - SFM_STOI_FIRST_BIN; ++c) {
      const double re = row[c], im = row[SK_NBIN + c];
      s += re * re + im * im;
    }
    out[(long long)(f0 + m0 + r) * SFM_STOI_BANDS + b] = (float)sqrt(s);
  }
}

// stoi_bands_kernel for the two signals ya, yb of the OPT-PCIRM search (pso.hip: the candidate's enhanced signal is ya + x yb), which
// share the clean signal's kept list.  Spectral frame m of ya + x yb is A + x B, so the energy of band j is P + 2 x Q + x^2 R with
// P = sum |A_k|^2, Q = sum Re(A_k conj B_k), R = sum |B_k|^2 over the band's bins: planes[frame_off[u] + m][3][15] in fp64 (the quadratic
// is evaluated at arbitrary x later; Q is formed from the fp64 products, never by a difference of rounded band rows).  Both tiles
// are rebuilt and windowed side by side (dynamic LDS: two A tiles), one B fragment of the DFT operand feeds both accumulator sets,
// which share their lane layout: a a, a b, b b are formed in registers and go through the one product tile, one plane after the other.
#define SK_PAIR_LDS (2 * SFM_STOI_ROW_TILE * SK_AS * (int)sizeof(double))
static_assert(2 * SK_AS >= SK_CS, "the product tile fits in the two A tiles");

__global__ __launch_bounds__(256) void stoi_bands_pair_kernel(const float* __restrict__ siga, const float* __restrict__ sigb,
                                                              const float* __restrict__ win, const float* __restrict__ dft,
                                                              const int* __restrict__ sig_off, const int* __restrict__ frame_off,
                                                              const int* __restrict__ src, const int* __restrict__ kept,
                                                              const int* __restrict__ tiles, double* __restrict__ planes) {
  extern __shared__ double pair_tile[];                     // the A tiles [2][16][257], then the products [16][433]
  __shared__ int stab[SFM_STOI_ROW_TILE + 2];               // src[m0 - 1 .. m0 + 16]
  double* tile = pair_tile;
  double* tile_b = pair_tile + SFM_STOI_ROW_TILE * SK_AS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = tiles[2 * blockIdx.x], m0 = tiles[2 * blockIdx.x + 1] * SFM_STOI_ROW_TILE;
  const int f0 = frame_off[u], K = kept[u], M = K - 1;      // M spectral frames: the last kept frame starts none
  if (m0 >= M) return;
  const float* xa = siga + sig_off[u];
  const float* xb = sigb + sig_off[u];
  if (tid < SFM_STOI_ROW_TILE + 2) {
    const int k = m0 - 1 + tid;
    stab[tid] = (k >= 0 && k < K) ? src[f0 + k] : 0;
  }
  __syncthreads();
  {
    const int n = tid, no = tid ^ SFM_STOI_HOP;
    const double wn = (double)win[n], wo = (double)win[no];
    for (int r = 0; r < SFM_STOI_ROW_TILE; ++r) {
      const int m = m0 + r;
      double za = 0.0, zb = 0.0;
      if (m < M) {
        const long long c = (long long)stab[r + 1] * SFM_STOI_HOP + n;
        double va = wn * (double)xa[c], vb = wn * (double)xb[c];
        if (n >= SFM_STOI_HOP) {                            // head of kept frame m + 1
          const long long o = (long long)stab[r + 2] * SFM_STOI_HOP + no;
          va += wo * (double)xa[o];
          vb += wo * (double)xb[o];
        } else if (m >= 1) {                                // tail of kept frame m - 1
          const long long o = (long long)stab[r] * SFM_STOI_HOP + no;
          va += wo * (double)xa[o];
          vb += wo * (double)xb[o];
        }
        za = wn * va;
        zb = wn * vb;
      }
      tile[r * SK_AS + n] = za;
      tile_b[r * SK_AS + n] = zb;
    }
  }
  __syncthreads();
  constexpr int NCT = SFM_STOI_DFT_COLS / 16;               // 27 column tiles: wave w takes w, w + 4, .. (7, 7, 7, 6)
  constexpr int NJ = (NCT + 3) / 4;
  f64x4 acca[NJ], accb[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acca[j] = accb[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  const double* apa = tile + (lane & 15) * SK_AS + (lane >> 4);
  const double* apb = tile_b + (lane & 15) * SK_AS + (lane >> 4);
  const float* bp = dft + (long long)(lane >> 4) * SFM_STOI_DFT_COLS + wave * 16 + (lane & 15);
#pragma unroll 2
  for (int ks = 0; ks < SFM_STOI_FRAME / 4; ++ks) {
    const double a = apa[4 * ks], b = apb[4 * ks];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (wave + 4 * j < NCT) {
        const double bv = (double)bp[(long long)(4 * ks) * SFM_STOI_DFT_COLS + 64 * j];
        acca[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acca[j], 0, 0, 0);
        accb[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, bv, accb[j], 0, 0, 0);
      }
    }
  }
  // rows and columns of this lane's four results, asked of the instruction as stoi_bands_kernel asks
  const double idx = (lane >> 4) == 0 ? (double)(lane & 15) : 0.0, one = (lane >> 4) == 0 ? 1.0 : 0.0;
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  const f64x4 drow = __builtin_amdgcn_mfma_f64_16x16x4f64(idx, one, zero, 0, 0, 0);
  const f64x4 dcol = __builtin_amdgcn_mfma_f64_16x16x4f64(one, idx, zero, 0, 0, 0);
#pragma unroll
  for (int pl = 0; pl < SFM_STOI_PLANES; ++pl) {
    __syncthreads();                                        // every wave has read its A fragments / the last plane's products
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (wave + 4 * j < NCT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = min(max((int)drow[r], 0), SFM_STOI_ROW_TILE - 1), col = min(max((int)dcol[r], 0), 15);
          const double l = pl == 2 ? accb[j][r] : acca[j][r], h = pl == 0 ? acca[j][r] : accb[j][r];
          tile[row * SK_CS + (wave + 4 * j) * 16 + col] = l * h;
        }
      }
    }
    __syncthreads();
    for (int it = tid; it < SFM_STOI_ROW_TILE * SFM_STOI_BANDS; it += 256) {
      const int r = it / SFM_STOI_BANDS, b = it - r * SFM_STOI_BANDS;
      if (m0 + r >= M) continue;
      const double* row = tile + r * SK_CS;
      double s = 0.0;
      for (int c = sk_edges[b] - SFM_STOI_FIRST_BIN; c < sk_edges[b + 1] - SFM_STOI_FIRST_BIN; ++c) s += row[c] + row[SK_NBIN + c];
      planes[((long long)(f0 + m0 + r) * SFM_STOI_PLANES + pl) * SFM_STOI_BANDS + b] = s;
    }
  }
}

// Step 0, the polyphase resampler: out sample n = t up + p of utterance u = sum_k in[t down + k - padl] taps[k][p] over the samples
// the utterance has, fp32 operands, the sum an fma chain in fp64 in k order, stored as fp32.  One thread per output sample.
__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ in, const float* __restrict__ taps,
                                                            const int* __restrict__ in_off, const int* __restrict__ in_len,
                                                            const int* __restrict__ out_off, const int* __restrict__ out_len,
                                                            float* __restrict__ out, int up, int down, int K, int padl) {
  const int u = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= out_len[u]) return;
  const int t = n / up, p = n - t * up, len = in_len[u];
  const float* x = in + in_off[u];
  const long long s0 = (long long)t * down - padl;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    const long long s = s0 + k;
    if (s >= 0 && s < len) acc = fma((double)x[s], (double)taps[k * up + p], acc);
  }
  out[(long long)out_off[u] + n] = (float)acc;
}

// Steps 4 and 5 for one utterance of M >= SFM_STOI_SEG spectral frames, by the whole workgroup: the band rows go through a ring in
// LDS, SFM_STOI_SEG_TILE segments per stage, each element fetched once through load(i, x, y), i = row * SFM_STOI_BANDS + band (x the
// clean value, y the other signal's, held as TY); a wave takes one segment at a time, one lane per band (STOI: scale, clip,
// correlate) or per band and then per frame (ESTOI: rows, then columns normalised); the segment values are added in segment order.
// -> the score, on thread 0.  The one statement of the segment arithmetic: stoi_segments_kernel and pso_fitness_taal_kernel call it.
template <typename T>
static __device__ __forceinline__ void sk_row_norm(const T (*ring)[SFM_STOI_BANDS], double (*out)[SFM_STOI_SEG], int r0, int lane) {
  double s = 0.0;
  for (int n = 0; n < SFM_STOI_SEG; ++n) s += (double)ring[(r0 + n) & (SK_RING - 1)][lane];
  const double mean = s / SFM_STOI_SEG;
  double ss = 0.0;
  for (int n = 0; n < SFM_STOI_SEG; ++n) {
    const double d = (double)ring[(r0 + n) & (SK_RING - 1)][lane] - mean;
    ss += d * d;
  }
  const double inv = 1.0 / (sqrt(ss) + SK_EPS);
  for (int n = 0; n < SFM_STOI_SEG; ++n) out[lane][n] = ((double)ring[(r0 + n) & (SK_RING - 1)][lane] - mean) * inv;
}

template <bool EXT, typename TY, typename LOAD>
static __device__ __forceinline__ double sk_score(int M, LOAD load) {
  __shared__ float ringx[SK_RING][SFM_STOI_BANDS];
  __shared__ TY ringy[SK_RING][SFM_STOI_BANDS];
  __shared__ double rows[EXT ? 4 : 1][2][SFM_STOI_BANDS][SFM_STOI_SEG];      // ESTOI: the row-normalised block of each wave
  __shared__ double segval[SFM_STOI_SEG_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nseg = M - SFM_STOI_SEG + 1;
  const double clip = 1.0 + 5.623413251903491;              // 1 + 10^(15/20)
  double acc = 0.0;
  int loaded = 0;
  for (int s0 = 0; s0 < nseg; s0 += SFM_STOI_SEG_TILE) {
    const int cnt = min(SFM_STOI_SEG_TILE, nseg - s0);
    const int need = s0 + cnt - 1 + SFM_STOI_SEG;            // rows [0, need) serve the segments up to s0 + cnt - 1; need <= M
    for (int i = loaded * SFM_STOI_BANDS + tid; i < need * SFM_STOI_BANDS; i += 256) {
      const int r = i / SFM_STOI_BANDS, b = i - r * SFM_STOI_BANDS;
      load(i, ringx[r & (SK_RING - 1)][b], ringy[r & (SK_RING - 1)][b]);
    }
    loaded = need;
    __syncthreads();
    for (int i0 = 0; i0 < cnt; i0 += 4) {
      const int i = i0 + wave;
      const bool active = i < cnt;
      const int r0 = s0 + i;                                 // the segment's first row
      double term = 0.0;
      if (!EXT) {
        if (active && lane < SFM_STOI_BANDS) {
          double sx2 = 0.0, sy2 = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ringx[(r0 + n) & (SK_RING - 1)][lane], yv = (double)ringy[(r0 + n) & (SK_RING - 1)][lane];
            sx2 += xv * xv;
            sy2 += yv * yv;
          }
          const double alpha = sqrt(sx2) / (sqrt(sy2) + SK_EPS);
          double sx = 0.0, sy = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ringx[(r0 + n) & (SK_RING - 1)][lane], yv = (double)ringy[(r0 + n) & (SK_RING - 1)][lane];
            sx += xv;
            sy += fmin(alpha * yv, xv * clip);
          }
          const double mx = sx / SFM_STOI_SEG, my = sy / SFM_STOI_SEG;
          double sxx = 0.0, syy = 0.0, sxy = 0.0;
          for (int n = 0; n < SFM_STOI_SEG; ++n) {
            const double xv = (double)ringx[(r0 + n) & (SK_RING - 1)][lane], yv = (double)ringy[(r0 + n) & (SK_RING - 1)][lane];
            const double dx = xv - mx, dy = fmin(alpha * yv, xv * clip) - my;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
          }
          term = sxy / ((sqrt(sxx) + SK_EPS) * (sqrt(syy) + SK_EPS));
        }
      } else {
        if (active && lane < SFM_STOI_BANDS) {
          sk_row_norm(ringx, rows[wave][0], r0, lane);
          sk_row_norm(ringy, rows[wave][1], r0, lane);
        }
        __syncthreads();
        if (active && lane < SFM_STOI_SEG) {
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
          term = sxy / ((sqrt(sxx) + SK_EPS) * (sqrt(syy) + SK_EPS)) / SFM_STOI_SEG;
        }
      }
      term = wave_sum_d(term);
      if (active && lane == 0) segval[i] = term;
      __syncthreads();                                      // (uniform: cnt is the workgroup's) rows[] and segval[] are free again
    }
    if (tid == 0)
      for (int i = 0; i < cnt; ++i) acc += segval[i];
    __syncthreads();
  }
  return EXT ? acc / nseg : acc / ((double)nseg * SFM_STOI_BANDS);
}

template <bool EXT>
__global__ __launch_bounds__(256) void stoi_segments_kernel(const float* __restrict__ xb, const float* __restrict__ yb,
                                                            const int* __restrict__ frame_off, const int* __restrict__ kept,
                                                            double* __restrict__ score) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const int M = kept[u] - 1;
  if (M < SFM_STOI_SEG) {
    if (tid == 0) score[u] = 1e-5;
    return;
  }
  const float* xr = xb + (long long)frame_off[u] * SFM_STOI_BANDS;
  const float* yr = yb + (long long)frame_off[u] * SFM_STOI_BANDS;
  const double s = sk_score<EXT, float>(M, [&](int i, float& x, float& y) {
    x = xr[i];
    y = yr[i];
  });
  if (tid == 0) score[u] = s;
}

// The fitness of the OPT-PCIRM search on this measure: one workgroup per (particle, utterance).  The enhanced signal of the candidate x
// is ya + x yb (pso.hip), every step before the band energies is linear in it, so band j of spectral frame m has the energy
// P + 2 x Q + x^2 R of stoi_bands_pair_kernel's planes: the row of the other signal is sqrt(max(., 0)) in fp64, formed while the ring is
// filled and never stored; the clean rows are sfm_stoi_bands' (fp32).  x is rounded to fp32 first: the mask array holds it so.
template <bool EXT>
__global__ __launch_bounds__(256) void pso_fitness_taal_kernel(const float* __restrict__ xb, const double* __restrict__ planes,
                                                               const int* __restrict__ frame_off, const int* __restrict__ kept,
                                                               const double* __restrict__ pos, const int* __restrict__ stopped,
                                                               double* __restrict__ fitness, int N) {
  const int p = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
  if (stopped[u]) return;
  const int M = kept[u] - 1;
  const long long q = (long long)u * N + p;
  if (M < SFM_STOI_SEG) {
    if (tid == 0) fitness[q] = 1e-5;
    return;
  }
  const double x = (double)(float)pos[q], x2 = 2.0 * x, xx = x * x;
  const float* xr = xb + (long long)frame_off[u] * SFM_STOI_BANDS;
  const double* pr = planes + (long long)frame_off[u] * (SFM_STOI_PLANES * SFM_STOI_BANDS);
  const double s = sk_score<EXT, double>(M, [&](int i, float& cx, double& y) {
    const int r = i / SFM_STOI_BANDS, b = i - r * SFM_STOI_BANDS;
    const double* e = pr + r * (SFM_STOI_PLANES * SFM_STOI_BANDS) + b;
    cx = xr[i];
    y = sqrt(fmax(e[0] + x2 * e[SFM_STOI_BANDS] + xx * e[2 * SFM_STOI_BANDS], 0.0));
  });
  if (tid == 0) fitness[q] = s;
}

extern "C" int sfm_stoi_keep(const float* sig, const float* win, const int* sig_off, const int* sig_len, const int* frame_off,
                             double* energy, int* src, int* kept, int B, void* stream) {
  if (!sig || !win || !sig_off || !sig_len || !frame_off || !energy || !src || !kept) return SFM_ERR_ARG;
  if (B <= 0) return SFM_ERR_SHAPE;
  SFM_LAUNCH(stoi_keep_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sig, win, sig_off, sig_len, frame_off, energy, src, kept);
  return SFM_OK;
}

extern "C" int sfm_stoi_bands(const float* sig0, const float* sig1, const float* win, const float* dft, const int* sig_off,
                              const int* frame_off, const int* src, const int* kept, const int* tiles, float* bands0, float* bands1,
                              int n_tiles, int nsig, void* stream) {
  if (!sig0 || !win || !dft || !sig_off || !frame_off || !src || !kept || !bands0) return SFM_ERR_ARG;
  if (nsig != 1 && nsig != 2) return SFM_ERR_SHAPE;
  if (nsig == 2 && (!sig1 || !bands1)) return SFM_ERR_ARG;
  if (n_tiles < 0 || n_tiles > 65535 * 1024) return SFM_ERR_SHAPE;
  if (n_tiles == 0) return SFM_OK;                          // no utterance has a spectral frame: an empty table has no address
  if (!tiles) return SFM_ERR_ARG;
  SFM_LAUNCH(stoi_bands_kernel, dim3(n_tiles, nsig), dim3(256), 0, (hipStream_t)stream, sig0, sig1, win, dft, sig_off, frame_off, src,
             kept, tiles, bands0, bands1);
  return SFM_OK;
}

extern "C" int sfm_stoi_bands_pair(const float* siga, const float* sigb, const float* win, const float* dft, const int* sig_off,
                                   const int* frame_off, const int* src, const int* kept, const int* tiles, double* planes,
                                   int n_tiles, void* stream) {
  if (!siga || !sigb || !win || !dft || !sig_off || !frame_off || !src || !kept || !planes) return SFM_ERR_ARG;
  if (n_tiles < 0 || n_tiles > 65535 * 1024) return SFM_ERR_SHAPE;
  if (n_tiles == 0) return SFM_OK;                          // no utterance has a spectral frame: an empty table has no address
  if (!tiles) return SFM_ERR_ARG;
  SFM_LAUNCH_LDS(stoi_bands_pair_kernel, dim3(n_tiles), dim3(256), SK_PAIR_LDS, (hipStream_t)stream, siga, sigb, win, dft, sig_off,
                 frame_off, src, kept, tiles, planes);
  return SFM_OK;
}

extern "C" int sfm_pso_fitness_taal(const float* xb, const double* planes, const int* frame_off, const int* kept, const double* pos,
                                    const int* stopped, double* fitness, int B, int N, int extended, void* stream) {
  if (!xb || !planes || !frame_off || !kept || !pos || !stopped || !fitness) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || N < 1 || N > SFM_PSO_MAX_PARTICLES || (extended != 0 && extended != 1)) return SFM_ERR_SHAPE;
  const dim3 grid((unsigned)N, (unsigned)B);
  if (extended)
    SFM_LAUNCH(pso_fitness_taal_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, xb, planes, frame_off, kept, pos, stopped, fitness,
               N);
  else
    SFM_LAUNCH(pso_fitness_taal_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, xb, planes, frame_off, kept, pos, stopped,
               fitness, N);
  return SFM_OK;
}

extern "C" int sfm_stoi_resample(const float* in, const float* taps, const int* in_off, const int* in_len, const int* out_off,
                                 const int* out_len, float* out, int B, int max_out_len, int up, int down, int K, int padl,
                                 void* stream) {
  if (!in || !taps || !in_off || !in_len || !out_off || !out_len || !out) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || max_out_len < 0 || up < 1 || down < 1 || up > SFM_STOI_MAX_RATE || down > SFM_STOI_MAX_RATE || K < 1 ||
      K > 2 * SFM_STOI_TAP_HALF * SFM_STOI_MAX_RATE + 1 || padl < 0 || padl >= K)
    return SFM_ERR_SHAPE;
  if (max_out_len == 0) return SFM_OK;
  SFM_LAUNCH(stoi_resample_kernel, dim3((max_out_len + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, in, taps, in_off, in_len,
             out_off, out_len, out, up, down, K, padl);
  return SFM_OK;
}

extern "C" int sfm_stoi_segments(const float* xb, const float* yb, const int* frame_off, const int* kept, double* score, int B,
                                 int extended, void* stream) {
  if (!xb || !yb || !frame_off || !kept || !score) return SFM_ERR_ARG;
  if (B <= 0 || (extended != 0 && extended != 1)) return SFM_ERR_SHAPE;
  if (extended) SFM_LAUNCH(stoi_segments_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, xb, yb, frame_off, kept, score);
  else SFM_LAUNCH(stoi_segments_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, xb, yb, frame_off, kept, score);
  return SFM_OK;
}
