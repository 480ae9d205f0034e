// sfm_mask_resynth: steps 2-4 of TrainingPipeline.enhance_signal (training/pipeline.py:877-934) for a zero-padded batch in one
// launch: the Hann STFT of the noisy signal, the np.interp of the C channel values of the mask onto the STFT bins, the masked irfft,
// the overlap-add and the division by the window sum.  The spectrum, the interpolated gain and the synthesis frames live in LDS and
// registers only.  Both transforms are exact-fp32 products on v_mfma_f32_32x32x2_f32 (an fmaf chain, as in framed_gemm.hip):
//   forward  X [R, NC]  = frames [R, frame] x Wf [FR, NC]        (analysis window folded in; rows frame .. FR zero)
//   inverse  y [R, FR]  = (X * g) [R, NC]   x Wi [NC, FR]        (irfft coefficients, crop and synthesis window folded in)
// The 2F columns of a spectrum row hold two that are identically zero (the imaginary parts of DC and Nyquist); the operands leave
// them out, so NC = n_fft rounded up to 32: column j < F is Re X[j], column F + k - 1 is Im X[k], 1 <= k <= F - 2.
//
// hop = frame / 2, so output hop h (samples [h hop, (h + 1) hop)) is the first half of frame h plus the second half of frame h - 1.
// Workgroup t of an utterance computes the R = SFM_RESYNTH_TILE_FRAMES frames f0 .. f0 + R - 1, f0 = t (R - 1), and owns the hops
// f0 + 1 .. f0 + R - 1 (t = 0: hop 0 as well); frame f0 is the one it computes again after its left neighbour.  The two halves of
// every frame go to two LDS planes, each word written by one lane, and the epilogue adds them: no atomics, one store per sample, and
// a sample's value depends on its utterance's samples and mask rows alone.  Frames from N_b = min(T_b, T_mask) on get the gain 0.
// 8 waves, two per SIMD: in the forward product a wave owns column blocks (both row blocks share its B fragment), in the inverse
// (row block, column block) pairs; B fragments come straight from global memory (the two operands are L2-resident), 16 k-steps ahead.
#include "sfm_common.h"

#define RS_R SFM_RESYNTH_TILE_FRAMES
#define RS_MS 65                      // LDS row stride of the mask rows (C <= 64)
#define RS_PF 16                      // k-steps of B fragments in flight
#define RS_THREADS 512                // 8 waves, two per SIMD
#define RS_WAVES (RS_THREADS / 64)
static_assert(SFM_RESYNTH_COL_ALIGN == 2 * RS_PF, "padded operand dimensions are whole chunks of k-steps");
static_assert(3 * (SFM_RESYNTH_MAX_FRAME / 2) <= RS_THREADS, "one thread per word of the 1 / wsum table");
static_assert(RS_R == 64, "two 32-row MFMA blocks per tile");
static_assert(SFM_RESYNTH_MAX_CHANNELS < RS_MS, "a mask row fits its LDS row");

struct ResynthParams {
  const float* noisy;
  const float* mask;
  const int* lengths;
  const float* Wf;
  const float* Wi;
  const int* tab_idx;
  const float* tab_wt;
  const float* inv_wsum;
  float* out;
  int B, L, T_mask, frame, hop, C, FK, NC, FR, tiles;
};

// words of dynamic LDS: signal rows (R + 1 hops, reused as the first-half plane), second-half plane, gained spectrum, mask rows,
// 1 / wsum
static inline long long resynth_lds_words(int hop, int NC) {
  const long long S = hop | 1;
  return (RS_R + 1) * S + RS_R * S + (long long)RS_R * (NC + 1) + RS_R * RS_MS + 3 * hop;
}

// NRB 32-row blocks of A (LDS, through a_at(row block, k)) times one 32-column block of B (global, row stride ldb), k < 2 ksteps,
// ksteps a multiple of RS_PF.  No branch inside: the B fragments of the next RS_PF k-steps are in flight while this chunk's MFMAs
// run (the last chunk loads itself again), and a chunk's A fragments are read from LDS ahead of its MFMAs.
template <int NRB, class AF>
__device__ __forceinline__ void rs_block(f32x16 (&acc)[NRB], const float* __restrict__ Bg, int ldb, int ksteps, int lane, AF a_at) {
#pragma unroll
  for (int j = 0; j < NRB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const float* bp = Bg + (long long)(lane >> 5) * ldb + (lane & 31);
  float cur[RS_PF], nxt[RS_PF];
#pragma unroll
  for (int i = 0; i < RS_PF; ++i) cur[i] = bp[(long long)2 * i * ldb];
  for (int k0 = 0; k0 < ksteps; k0 += RS_PF) {
    const int kn = min(k0 + RS_PF, ksteps - RS_PF);
#pragma unroll
    for (int i = 0; i < RS_PF; ++i) nxt[i] = bp[(long long)2 * (kn + i) * ldb];
    float a[NRB][RS_PF];
#pragma unroll
    for (int i = 0; i < RS_PF; ++i)
#pragma unroll
      for (int j = 0; j < NRB; ++j) a[j][i] = a_at(j, 2 * (k0 + i) + (lane >> 5));
#pragma unroll
    for (int i = 0; i < RS_PF; ++i)
#pragma unroll
      for (int j = 0; j < NRB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][i], cur[i], acc[j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < RS_PF; ++i) cur[i] = nxt[i];
  }
}

__global__ __launch_bounds__(RS_THREADS) void mask_resynth_kernel(ResynthParams p) {
  extern __shared__ float rs_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / p.tiles, t = blockIdx.x - b * p.tiles;
  const int hop = p.hop, S = hop | 1;
  float* sigL = rs_lds;                                   // [R + 1][S] hop rows of the signal; after the forward product:
  float* olaA = rs_lds;                                   // [R][S] first half of frame r (hop f0 + r)
  float* olaB = sigL + (RS_R + 1) * S;                    // [R][S] second half of frame r (hop f0 + r + 1)
  float* Xs = olaB + RS_R * S;                            // [R][NC + 1] spectrum times gain
  float* Ms = Xs + RS_R * (p.NC + 1);                     // [R][65] mask rows
  float* Ws = Ms + RS_R * RS_MS;                          // [3][hop] 1 / wsum: first hop, interior, last covered hop
  const int XS = p.NC + 1;

  int Lb = p.lengths ? p.lengths[b] : p.L;
  Lb = Lb < 0 ? 0 : (Lb > p.L ? p.L : Lb);
  const int Tb = Lb >= p.frame ? (Lb - p.frame) / hop + 1 : 0;
  const int Nb = Tb < p.T_mask ? Tb : p.T_mask;
  const int f0 = t * (RS_R - 1);
  const float* sg = p.noisy + (long long)b * p.L;
  float* og = p.out + (long long)b * p.L;
  const int own0 = t == 0 ? 0 : 1;                        // first owned hop, tile-local
  const int nown = (RS_R - own0) * hop;                   // owned samples

  if (f0 >= Nb) {                                         // no frame of this tile is live (workgroup-uniform): zeros
    for (int i = tid; i < nown; i += RS_THREADS) {
      const long long s = (long long)(f0 + own0) * hop + i;
      if (s < p.L) og[s] = 0.f;
    }
    return;
  }

  // ---- stage: R + 1 hops of the signal (0 from the utterance's length on), R mask rows (0 from frame N_b on), 1 / wsum.  All of a
  //      thread's loads are issued before its first LDS store: one round trip to memory, not one per element ----
  {
    constexpr int NS = ((RS_R + 1) * (SFM_RESYNTH_MAX_FRAME / 2) + RS_THREADS - 1) / RS_THREADS, NM = RS_R * 64 / RS_THREADS;
    float vs[NS], vm[NM];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = tid + u * RS_THREADS;
      const long long s = (long long)f0 * hop + i;
      vs[u] = (i < (RS_R + 1) * hop && s < Lb) ? sg[s] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NM; ++u) {
      const int i = tid + u * RS_THREADS, r = i >> 6, c = i & 63, n = f0 + r;
      vm[u] = (n < Nb && c < p.C) ? p.mask[((long long)b * p.T_mask + n) * p.C + c] : 0.f;
    }
    const float vw = tid < 3 * hop ? p.inv_wsum[tid] : 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = tid + u * RS_THREADS, h = i / hop;
      if (i < (RS_R + 1) * hop) sigL[h * S + i - h * hop] = vs[u];
    }
#pragma unroll
    for (int u = 0; u < NM; ++u) {
      const int i = tid + u * RS_THREADS;
      Ms[(i >> 6) * RS_MS + (i & 63)] = vm[u];
    }
    if (tid < 3 * hop) Ws[tid] = vw;
  }
  __syncthreads();

  // ---- forward: X = frames x Wf, times the interpolated gain on the way into the inverse product's A operand ----
  const int l31 = lane & 31;
  for (int cb = wave; cb < p.NC / 32; cb += RS_WAVES) {
    f32x16 acc[2];
    rs_block<2>(acc, p.Wf + cb * 32, p.NC, p.FK / 2, lane, [&](int j, int k) {
      k = min(k, p.frame - 1);                            // rows frame .. FK of Wf are zero: any finite sample of the frame serves
      const int hr = k >= hop ? 1 : 0;
      return sigL[(j * 32 + l31 + hr) * S + k - hr * hop];
    });
    const int col = cb * 32 + l31;
    const int ci = min(max(p.tab_idx[col], 0), p.C - 2);
    const float w1 = p.tab_wt[col], w0 = 1.f - w1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float lo[16], hi[16];                               // (all mask reads ahead of the stores: the two LDS regions do not alias)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = j * 32 + mfma_row(r, lane);
        lo[r] = Ms[row * RS_MS + ci];
        hi[r] = Ms[row * RS_MS + ci + 1];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = j * 32 + mfma_row(r, lane);
        Xs[row * XS + col] = acc[j][r] * __builtin_fmaf(w1, hi[r], w0 * lo[r]);
      }
    }
  }
  __syncthreads();

  // ---- inverse: y = Xs x Wi; the halves of every frame go to the two overlap-add planes ----
  const int ncbi = p.FR / 32;
  for (int pr = wave; pr < 2 * ncbi; pr += RS_WAVES) {
    const int rb = pr / ncbi, cb = pr - rb * ncbi;
    f32x16 acc[1];
    rs_block<1>(acc, p.Wi + cb * 32, p.FR, p.NC / 2, lane, [&](int, int k) { return Xs[(rb * 32 + l31) * XS + k]; });
    const int j = cb * 32 + l31;
    if (j < p.frame) {
      float* dst = j < hop ? olaA + j : olaB + (j - hop);
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(rb * 32 + mfma_row(r, lane)) * S] = acc[0][r];
    }
  }
  __syncthreads();

  // ---- epilogue: hop h = first half of frame h + second half of frame h - 1, over the window sum of the frames that cover it ----
  for (int i = tid; i < nown; i += RS_THREADS) {
    const int hl = own0 + i / hop, j = i % hop;           // tile-local hop, sample of the hop
    const int hg = f0 + hl;
    const long long s = (long long)hg * hop + j;
    if (s >= p.L) continue;
    float v = 0.f;
    if (hg <= Nb) {
      const float a = olaA[hl * S + j];
      const float sum = hl > 0 ? olaB[(hl - 1) * S + j] + a : a;
      const int row = hg == 0 ? 0 : (hg == Nb ? 2 : 1);   // first hop of the utterance, interior, last covered hop
      v = sum * Ws[row * hop + j];
    }
    og[s] = v;
  }
}

extern "C" int sfm_mask_resynth(const float* noisy, const float* mask, const int* lengths, const float* Wf, const float* Wi,
                                const int* tab_idx, const float* tab_wt, const float* inv_wsum, float* out, int B, int L,
                                int T_mask, int frame, int hop, int n_fft, int C, void* stream) {
  if (!noisy || !mask || !Wf || !Wi || !tab_idx || !tab_wt || !inv_wsum || !out) return SFM_ERR_ARG;
  if (B <= 0 || L <= 0 || T_mask <= 0 || hop <= 0 || frame <= 0 || n_fft <= 0) return SFM_ERR_SHAPE;
  if (hop * 2 != frame || frame > n_fft || (n_fft & 1) || C > SFM_RESYNTH_MAX_CHANNELS || C < 2) return SFM_ERR_SHAPE;
  if (n_fft > SFM_RESYNTH_MAX_NFFT || frame > SFM_RESYNTH_MAX_FRAME) return SFM_ERR_SHAPE;
  ResynthParams p;
  p.noisy = noisy; p.mask = mask; p.lengths = lengths; p.Wf = Wf; p.Wi = Wi; p.tab_idx = tab_idx; p.tab_wt = tab_wt;
  p.inv_wsum = inv_wsum; p.out = out;
  p.B = B; p.L = L; p.T_mask = T_mask; p.frame = frame; p.hop = hop; p.C = C;
  p.NC = (n_fft + SFM_RESYNTH_COL_ALIGN - 1) / SFM_RESYNTH_COL_ALIGN * SFM_RESYNTH_COL_ALIGN;
  p.FR = (frame + SFM_RESYNTH_COL_ALIGN - 1) / SFM_RESYNTH_COL_ALIGN * SFM_RESYNTH_COL_ALIGN;
  p.FK = p.FR;
  const long long hops = ((long long)L + hop - 1) / hop;              // every hop that holds a sample of the [B, L] output is owned
  const long long tiles = hops > 1 ? (hops - 1 + RS_R - 2) / (RS_R - 1) : 1;
  if (tiles * B > 2147483647LL) return SFM_ERR_SHAPE;
  p.tiles = (int)tiles;
  const int lds = (int)(resynth_lds_words(hop, p.NC) * 4);
  SFM_LAUNCH_LDS(mask_resynth_kernel, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), lds, (hipStream_t)stream, p);
  return SFM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sfm_mask_resynth_bwd: the adjoint of sfm_mask_resynth with respect to the mask.  The forward is linear in the mask, so the
// cotangent needs the noisy signal and dout alone:
//   dy_n[j]   = dout[n hop + j] / wsum(n hop + j)              the forward's row choice: first hop, interior, last covered hop
//   X  [R, NC] = frames [R, frame] x Wf  [FR, NC]              the forward's own first product
//   dZ [R, NC] = dy     [R, frame] x WiT [FR, NC]              Wi transposed: the same shape, so rs_block<2> serves both
//   P = X * dZ;   dg[k] = P[k] + P[F + k - 1] (the Im column exists for 1 <= k <= F - 2)
//   dmask[n, c] = sum_{idx[k] == c - 1} wt[k] dg[k] + sum_{idx[k] == c} (1 - wt[k]) dg[k]
// idx ascends with k, so both sums run over contiguous bins: chan_bins[c] .. chan_bins[c + 1] - 1 are the bins with idx == c.
// A dmask row belongs to one frame, so workgroup t of an utterance computes the R = SFM_RESYNTH_BWD_TILE_FRAMES frames from t R on
// and shares none with its neighbours.  The R + 1 hop rows of the signal and of dout / wsum (the quotient is formed on the way into
// LDS, from the table in global memory: one round trip, no table plane) are staged, a wave owns column blocks and both row blocks so
// that X and dZ of an element meet in its registers, and only P goes to LDS.  The fold turns the tile: lane = row, a wave walks
// channels, so the trip count and the table words are wave-uniform and the reads of P (odd row stride) conflict-free; the R x C
// result goes through LDS (over the dead signal planes) to stores with c fastest.  No atomics; rows from N_b on are written as 0;
// dout is not read from min(L_b, (N_b + 1) hop) on.
#define RSB_R SFM_RESYNTH_BWD_TILE_FRAMES
static_assert(RSB_R == 64, "two 32-row MFMA blocks per tile, one fold row per lane");

struct ResynthBwdParams {
  const float* noisy;
  const float* dout;
  const int* lengths;
  const float* Wf;
  const float* WiT;
  const float* tab_wt;
  const float* inv_wsum;
  const int* chan_bins;
  float* dmask;
  int B, L, T_mask, frame, hop, C, F, FK, NC, tiles;
};

// words of dynamic LDS: two signal planes of R + 1 hop rows (reused as the [R][65] result tile), the plane of P
static inline long long resynth_bwd_lds_words(int hop, int NC) {
  const long long S = hop | 1, planes = 2 * (RSB_R + 1) * S, tile = (long long)RSB_R * RS_MS;
  return (planes > tile ? planes : tile) + (long long)RSB_R * (NC + 1);
}

__global__ __launch_bounds__(RS_THREADS) void mask_resynth_bwd_kernel(ResynthBwdParams p) {
  extern __shared__ float rs_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / p.tiles, t = blockIdx.x - b * p.tiles;
  const int hop = p.hop, S = hop | 1, XS = p.NC + 1;
  const int plane = (RSB_R + 1) * S;
  float* sigL = rs_lds;                                   // [R + 1][S] hop rows of the signal
  float* dyL = sigL + plane;                              // [R + 1][S] hop rows of dout / wsum
  float* Ds = rs_lds;                                     // [R][65] the tile of dmask, once both products are done
  float* Ps = rs_lds + max(2 * plane, RSB_R * RS_MS);     // [R][NC + 1] X * dZ

  int Lb = p.lengths ? p.lengths[b] : p.L;
  Lb = Lb < 0 ? 0 : (Lb > p.L ? p.L : Lb);
  const int Tb = Lb >= p.frame ? (Lb - p.frame) / hop + 1 : 0;
  const int Nb = Tb < p.T_mask ? Tb : p.T_mask;
  const int f0 = t * RSB_R;
  const int nrow = min(RSB_R, p.T_mask - f0);             // rows of dmask this tile owns (tiles = ceil(T_mask / R): at least 1)
  float* dg = p.dmask + ((long long)b * p.T_mask + f0) * p.C;

  if (f0 >= Nb) {                                         // no frame of this tile is live (workgroup-uniform): zeros
    for (int i = tid; i < nrow * p.C; i += RS_THREADS) dg[i] = 0.f;
    return;
  }

  // ---- stage: R + 1 hops of the signal (0 from L_b on) and of dout / wsum (0 from min(L_b, (N_b + 1) hop) on: never read there).
  //      All of a thread's loads are issued before its first LDS store ----
  {
    constexpr int NS = ((RSB_R + 1) * (SFM_RESYNTH_MAX_FRAME / 2) + RS_THREADS - 1) / RS_THREADS;
    const float* sg = p.noisy + (long long)b * p.L;
    const float* dd = p.dout + (long long)b * p.L;
    const long long live = (long long)(Nb + 1) * hop;
    const long long lim = live < Lb ? live : (long long)Lb;
    float vs[NS], vd[NS], vw[NS];
    int at[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int i = tid + u * RS_THREADS, h = i / hop, j = i - h * hop, hg = f0 + h;
      const bool in = i < (RSB_R + 1) * hop;
      const long long s = (long long)f0 * hop + i;
      const int row = hg == 0 ? 0 : (hg == Nb ? 2 : 1);   // first hop of the utterance, interior, last covered hop
      at[u] = in ? h * S + j : -1;
      vs[u] = (in && s < Lb) ? sg[s] : 0.f;
      vd[u] = (in && s < lim) ? dd[s] : 0.f;
      vw[u] = in ? p.inv_wsum[row * hop + j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < NS; ++u)
      if (at[u] >= 0) {
        sigL[at[u]] = vs[u];
        dyL[at[u]] = vd[u] * vw[u];
      }
  }
  __syncthreads();

  // ---- both products, then P = X * dZ ----
  const int l31 = lane & 31;
  for (int cb = wave; cb < p.NC / 32; cb += RS_WAVES) {
    f32x16 ax[2], az[2];
    auto rows_of = [&](const float* pl) {
      return [=](int j, int k) {
        k = min(k, p.frame - 1);                          // rows frame .. FK of Wf and WiT are zero: any finite value serves
        const int hr = k >= hop ? 1 : 0;
        return pl[(j * 32 + l31 + hr) * S + k - hr * hop];
      };
    };
    rs_block<2>(ax, p.Wf + cb * 32, p.NC, p.FK / 2, lane, rows_of(sigL));
    rs_block<2>(az, p.WiT + cb * 32, p.NC, p.FK / 2, lane, rows_of(dyL));
    const int col = cb * 32 + l31;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) Ps[(j * 32 + mfma_row(r, lane)) * XS + col] = ax[j][r] * az[j][r];
  }
  __syncthreads();

  // ---- channel fold: lane = row, the wave's channel is uniform; ascending bins, Re and Im column of each ----
  {
    const int wv = __builtin_amdgcn_readfirstlane(wave), F = p.F;
    const float* pr = Ps + lane * XS;
    auto bin = [&](int k) { return (k >= 1 && k <= F - 2) ? pr[k] + pr[F + k - 1] : pr[k]; };
    for (int c = wv; c < p.C; c += RS_WAVES) {
      const int k1 = min(max(p.chan_bins[c], 0), F), k2 = min(max(p.chan_bins[c + 1], k1), F);
      float acc = 0.f;
      if (c > 0) {
        const int k0 = min(max(p.chan_bins[c - 1], 0), k1);
        for (int k = k0; k < k1; ++k) acc = __builtin_fmaf(p.tab_wt[k], bin(k), acc);
      }
      for (int k = k1; k < k2; ++k) acc = __builtin_fmaf(1.f - p.tab_wt[k], bin(k), acc);
      Ds[lane * RS_MS + c] = f0 + lane < Nb ? acc : 0.f;
    }
  }
  __syncthreads();
  for (int i = tid; i < nrow * 64; i += RS_THREADS) {
    const int r = i >> 6, c = i & 63;
    if (c < p.C) dg[r * p.C + c] = Ds[r * RS_MS + c];
  }
}

extern "C" int sfm_mask_resynth_bwd(const float* noisy, const float* dout, const int* lengths, const float* Wf, const float* WiT,
                                    const float* tab_wt, const float* inv_wsum, const int* chan_bins, float* dmask, int B, int L,
                                    int T_mask, int frame, int hop, int n_fft, int C, void* stream) {
  if (!noisy || !dout || !Wf || !WiT || !tab_wt || !inv_wsum || !chan_bins || !dmask) return SFM_ERR_ARG;
  if (B <= 0 || L <= 0 || T_mask <= 0 || hop <= 0 || frame <= 0 || n_fft <= 0) return SFM_ERR_SHAPE;
  if (hop * 2 != frame || frame > n_fft || (n_fft & 1) || C > SFM_RESYNTH_MAX_CHANNELS || C < 2) return SFM_ERR_SHAPE;
  if (n_fft > SFM_RESYNTH_MAX_NFFT || frame > SFM_RESYNTH_MAX_FRAME) return SFM_ERR_SHAPE;
  ResynthBwdParams p;
  p.noisy = noisy; p.dout = dout; p.lengths = lengths; p.Wf = Wf; p.WiT = WiT; p.tab_wt = tab_wt; p.inv_wsum = inv_wsum;
  p.chan_bins = chan_bins; p.dmask = dmask;
  p.B = B; p.L = L; p.T_mask = T_mask; p.frame = frame; p.hop = hop; p.C = C; p.F = n_fft / 2 + 1;
  p.NC = (n_fft + SFM_RESYNTH_COL_ALIGN - 1) / SFM_RESYNTH_COL_ALIGN * SFM_RESYNTH_COL_ALIGN;
  p.FK = (frame + SFM_RESYNTH_COL_ALIGN - 1) / SFM_RESYNTH_COL_ALIGN * SFM_RESYNTH_COL_ALIGN;
  const long long tiles = ((long long)T_mask + RSB_R - 1) / RSB_R;
  if (tiles * B > 2147483647LL) return SFM_ERR_SHAPE;
  p.tiles = (int)tiles;
  const int lds = (int)(resynth_bwd_lds_words(hop, p.NC) * 4);
  SFM_LAUNCH_LDS(mask_resynth_bwd_kernel, dim3((unsigned)(tiles * B)), dim3(RS_THREADS), lds, (hipStream_t)stream, p);
  return SFM_OK;
}
