// Stage objectives of the curriculum (training/losses.py:22-143): MSEMaskLoss and PerceptualSTOILoss, forward and - when the
// caller asks - the gradient to the enhanced side, in one launch each.  Sums over workgroups go through one partial per
// workgroup and the ordered fold of reduce.hip: no floating-point atomics, loss and gradient are the same bits from run to run.
//
// sfm_pstoi_loss: one workgroup per (utterance, segment of FL frames).
//   stage   the segment of both spectrograms into LDS (channels-last pairs: one contiguous run of FL * F floats per array,
//           16-byte loads between a scalar head and tail, magnitude sqrt(re^2 + im^2 + 1e-8) taken on the way;
//           [B, F, T] magnitudes: F runs of FL floats, one half-wave per run), and the band matrix as a dense operand
//   envelop one wave per 4 bands: lanes 0-31 hold the enhanced frames, lanes 32-63 the clean ones (so FL <= 32), each lane
//           runs the F-long dot products of its frame with 4 band rows (one 16-byte LDS read of the transposed matrix per bin)
//   stats   the halves swap envelopes; means, energies, clip factor, correlation and d corr / d envelope by xor-butterflies
//           inside a half-wave (a fixed order); both halves compute the same numbers
//   grad    d spec[f][t] = sum_k W[k][f] * d env[k][t] for EVERY bin and frame of the segment (bins of no band get 0), times
//           re / mag, im / mag in the pair form (re, im read again: they were this workgroup's last loads); the workgroup of an
//           utterance's last segment also zeroes the frames t >= S * FL that no segment uses.
#include "sfm_common.h"

#define PST_EPS 1e-8f
static_assert(SFM_PSTOI_MAX_FRAME_LEN == 32, "a segment's frames are the lanes of a half-wave (pstoi_kernel)");

// sum over the 32 lanes of a half-wave, the same value (bit for bit) in each of them
static __device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
static __device__ __forceinline__ float pst_mag(float re, float im) { return sqrtf(re * re + im * im + PST_EPS); }

// LDS (floats): WT [F][NBp] | E [xsz] | C [xsz] | G [NBp][32] | CORR [NBp] | W [NB][F] (channels-last gradient only)
static inline int pst_ld(int layout, int F, int FL) { return layout ? (F | 1) : (FL | 1); }
static inline int pst_xsz(int layout, int F, int FL) { return ((layout ? FL : F) * pst_ld(layout, F, FL) + 4 + 3) & ~3; }

// LAYOUT 0: e0 / c0 magnitudes [B, F, T], g0 likewise.  LAYOUT 1: (e0, e1) / (c0, c1) = (real, imag) [B, T, F], (g0, g1) likewise.
template <int LAYOUT, bool GRAD>
__global__ __launch_bounds__(256) void pstoi_kernel(const float* __restrict__ e0, const float* __restrict__ e1,
                                                    const float* __restrict__ c0, const float* __restrict__ c1,
                                                    const float* __restrict__ bw, float* __restrict__ g0, float* __restrict__ g1,
                                                    double* __restrict__ part, int T, int F, int NB, int FL, int S, float clip,
                                                    float gscale, int vec) {
  extern __shared__ __align__(16) float pst_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NBp = (NB + 3) & ~3;
  const int b = blockIdx.x / S, s = blockIdx.x - b * S;
  const int ld = LAYOUT ? (F | 1) : (FL | 1);                      // odd: 32 consecutive rows fall on 32 different banks
  const int xsz = ((LAYOUT ? FL : F) * ld + 4 + 3) & ~3;
  float* WT = pst_lds;
  float* E = WT + F * NBp;
  float* C = E + xsz;
  float* G = C + xsz;
  float* CORR = G + NBp * 32;
  float* W = CORR + NBp;

  for (int i = tid; i < NB * F; i += 256) {
    const int k = i / F, f = i - k * F;
    const float w = bw[i];
    WT[f * NBp + k] = w;
    if (LAYOUT && GRAD) W[i] = w;
  }
  if (NBp > NB) {
    const int pad = NBp - NB;
    for (int i = tid; i < F * pad; i += 256) {
      const int f = i / pad;
      WT[f * NBp + NB + (i - f * pad)] = 0.f;
    }
  }

  // ---- stage the segment ----
  const int n = FL * F;                                            // channels-last: the run's length
  const long long base = ((long long)b * T + (long long)s * FL) * F;   // ... and its first element
  const bool flat = LAYOUT && ld == F;                             // the run is copied as it lies (F odd)
  const bool v4 = flat && vec;
  const int xoff = v4 ? (int)(base & 3) : 0;                       // LDS index = global index mod 4: aligned 16-byte LDS accesses
  int head = 0, nq = 0;
  if (v4) {
    head = (int)((4 - (base & 3)) & 3);
    if (head > n) head = n;
    nq = (n - head) >> 2;
  }
  const int tail0 = head + 4 * nq;
  if (LAYOUT) {
    if (flat) {
      for (int q = tid; q < nq; q += 256) {
        const int j = head + 4 * q;
        const f32x4 a = *reinterpret_cast<const f32x4*>(e0 + base + j), bi = *reinterpret_cast<const f32x4*>(e1 + base + j);
        const f32x4 c = *reinterpret_cast<const f32x4*>(c0 + base + j), d = *reinterpret_cast<const f32x4*>(c1 + base + j);
        f32x4 me, mc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          me[i] = pst_mag(a[i], bi[i]);
          mc[i] = pst_mag(c[i], d[i]);
        }
        *reinterpret_cast<f32x4*>(E + xoff + j) = me;
        *reinterpret_cast<f32x4*>(C + xoff + j) = mc;
      }
      if (tid < head) {
        E[xoff + tid] = pst_mag(e0[base + tid], e1[base + tid]);
        C[xoff + tid] = pst_mag(c0[base + tid], c1[base + tid]);
      }
      for (int j = tail0 + tid; j < n; j += 256) {
        E[xoff + j] = pst_mag(e0[base + j], e1[base + j]);
        C[xoff + j] = pst_mag(c0[base + j], c1[base + j]);
      }
    } else {
      for (int j = tid; j < n; j += 256) {
        const int t = j / F, f = j - t * F;
        E[t * ld + f] = pst_mag(e0[base + j], e1[base + j]);
        C[t * ld + f] = pst_mag(c0[base + j], c1[base + j]);
      }
    }
  } else {
    for (int i = tid; i < F * 32; i += 256) {
      const int f = i >> 5, t = i & 31;
      if (t < FL) {
        const long long o = ((long long)b * F + f) * T + (long long)s * FL + t;
        E[f * ld + t] = e0[o];
        C[f * ld + t] = c0[o];
      }
    }
  }
  __syncthreads();

  // ---- envelopes and per-band statistics ----
  {
    const int half = lane >> 5, t = lane & 31, tt = t < FL ? t : FL - 1;
    const bool live = t < FL;
    const float* X = half ? C : E;
    const int x0 = LAYOUT ? xoff + tt * ld : tt, xs = LAYOUT ? 1 : ld;
    const float fl = (float)FL;
    for (int grp = wave; grp < (NBp >> 2); grp += 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* wt = WT + 4 * grp;
#pragma unroll 4
      for (int f = 0; f < F; ++f) {
        const float x = X[x0 + f * xs];
        const f32x4 w = *reinterpret_cast<const f32x4*>(wt + f * NBp);
        acc += w * x;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * grp + j;
        if (k >= NB) break;                                        // (the same in every lane)
        const float mine = live ? acc[j] : 0.f;
        const float other = __shfl_xor(mine, 32, 64);
        const float e = half ? other : mine, c = half ? mine : other;
        const float me = half_sum(e) / fl, mc = half_sum(c) / fl;
        const float ez = live ? e - me : 0.f, cz = live ? c - mc : 0.f;
        const float cc = half_sum(cz * cz), ee = half_sum(ez * ez);
        const float cE = sqrtf(cc + PST_EPS), eE = sqrtf(ee + PST_EPS);
        const float r = clip * cE / (eE + PST_EPS);
        const bool clipped = r < 1.f;
        const float sc = clipped ? r : 1.f;
        const float ep = ez * sc;
        const float N = half_sum(cz * ep), pp = half_sum(ep * ep);
        const float n2 = sqrtf(pp + PST_EPS);
        const float D = cE * n2 + PST_EPS;
        if (lane == 0) CORR[k] = N / D;
        if (GRAD) {
          // corr = N / D: H = d corr / d e' (e' = sc * e); clipped: sc = clip * cE / (eE + 1e-8) moves with e as well,
          // d sc / d e_t = q * e_t, so d corr / d e_t = sc * H_t + q * e_t * sum_u H_u e_u; then back through the mean removal
          const float H = cz / D - (N * cE / (n2 * D * D)) * ep;
          const float he = half_sum(H * ez);
          const float q = clipped ? -sc / ((eE + PST_EPS) * eE) : 0.f;
          float Gt = sc * H + q * he * ez;
          Gt -= half_sum(Gt) / fl;
          if (half == 0) G[k * 32 + t] = live ? Gt * gscale : 0.f;
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < NB; ++k) sum += (double)CORR[k];
    part[blockIdx.x] = sum;
  }
  if (!GRAD) return;

  // ---- gradient: every element of the segment, and the unused tail frames of the utterance ----
  const int tail = s == S - 1 ? T - S * FL : 0;                    // < FL
  if (LAYOUT) {
    // d |spec| into E's place (the envelopes are done with it), in the order of the run
    {
      const int dq = 256 / F, dr = 256 - dq * F;                   // (t, f) of j + 256 from those of j: no division per element
      int t = tid / F, f = tid - t * F;
      for (int j = tid; j < n; j += 256) {
        float d = 0.f;
        for (int k = 0; k < NB; ++k) d += W[k * F + f] * G[k * 32 + t];
        E[flat ? xoff + j : t * ld + f] = d;
        t += dq;
        f += dr;
        if (f >= F) {
          f -= F;
          ++t;
        }
      }
    }
    __syncthreads();
    if (flat) {
      for (int q = tid; q < nq; q += 256) {
        const int j = head + 4 * q;
        const f32x4 d = *reinterpret_cast<const f32x4*>(E + xoff + j);
        const f32x4 a = *reinterpret_cast<const f32x4*>(e0 + base + j), bi = *reinterpret_cast<const f32x4*>(e1 + base + j);
        f32x4 dr, di;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float m = pst_mag(a[i], bi[i]);
          dr[i] = d[i] * a[i] / m;
          di[i] = d[i] * bi[i] / m;
        }
        *reinterpret_cast<f32x4*>(g0 + base + j) = dr;
        *reinterpret_cast<f32x4*>(g1 + base + j) = di;
      }
    }
    for (int j = tid; j < n; j += 256) {
      if (flat && j >= head && j < tail0) continue;
      const int t = j / F, f = j - t * F;
      const float d = E[flat ? xoff + j : t * ld + f];
      const float re = e0[base + j], im = e1[base + j], m = pst_mag(re, im);
      g0[base + j] = d * re / m;
      g1[base + j] = d * im / m;
    }
    const long long tb = base + n;
    for (int j = tid; j < tail * F; j += 256) {
      g0[tb + j] = 0.f;
      g1[tb + j] = 0.f;
    }
  } else {
    for (int i = tid; i < F * 32; i += 256) {
      const int f = i >> 5, t = i & 31;
      const long long row = ((long long)b * F + f) * T;
      if (t < FL) {
        float d = 0.f;
        for (int k = 0; k < NB; ++k) d += WT[f * NBp + k] * G[k * 32 + t];
        g0[row + (long long)s * FL + t] = d;
      }
      if (t < tail) g0[row + (long long)S * FL + t] = 0.f;
    }
  }
}

// out = (float)(sum * scale)
__global__ void scaled_sum_kernel(const double* __restrict__ sum, double scale, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (float)(sum[0] * scale);
}

// one partial per workgroup: sum (p - t)^2 in double; grad (or NULL) = (p - t) * gs, formed in double and rounded once
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ grad,
                                                  double* __restrict__ part, long long n, double gs) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double d = (double)p[i] - (double)t[i];
    acc += d * d;
    if (grad) grad[i] = (float)(d * gs);
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// loss[0] = -mean over (B, NB, S = T / frame_len) of the band / segment correlations; g0 (, g1) != NULL: d loss / d enhanced,
// every element written.  ws: sfm_pstoi_loss_ws_doubles doubles of scratch (one partial per workgroup, then their sum).
static long long pstoi_parts(int B, int T, int frame_len) { return (long long)B * (T / frame_len); }
extern "C" long long sfm_pstoi_loss_ws_doubles(int B, int T, int frame_len) {
  return B > 0 && T > 0 && frame_len > 0 ? pstoi_parts(B, T, frame_len) + 1 : 0;
}
extern "C" int sfm_pstoi_loss(const float* e0, const float* e1, const float* c0, const float* c1, const float* band_w,
                              float* loss, float* g0, float* g1, double* ws, int B, int T, int F, int NB, int frame_len,
                              float beta_db, int layout, void* stream) {
  if (!e0 || !c0 || !band_w || !loss || !ws || (layout != 0 && layout != 1)) return SFM_ERR_ARG;
  if (layout == 1 && (!e1 || !c1 || (g0 != nullptr) != (g1 != nullptr))) return SFM_ERR_ARG;
  if (layout == 0 && g1) return SFM_ERR_ARG;
  if (B <= 0 || F < 1 || F > SFM_PSTOI_MAX_BINS || NB < 1 || NB > SFM_PSTOI_MAX_BANDS || frame_len < SFM_PSTOI_MIN_FRAME_LEN ||
      frame_len > SFM_PSTOI_MAX_FRAME_LEN || T < frame_len)
    return SFM_ERR_SHAPE;
  const int FL = frame_len, S = T / FL;
  const long long parts = pstoi_parts(B, T, FL);
  if (parts > 2147483647LL) return SFM_ERR_SHAPE;
  const int NBp = (NB + 3) & ~3;
  const bool grad = g0 != nullptr;
  const int lds = (F * NBp + 2 * pst_xsz(layout, F, FL) + NBp * 32 + NBp + (layout && grad ? NB * F : 0)) * (int)sizeof(float);
  const double count = (double)parts * NB;
  const float clip = (float)pow(10.0, (double)beta_db / 20.0);
  const float gscale = (float)(-1.0 / count);
  const int vec = layout == 1 && al16(e0) && al16(e1) && al16(c0) && al16(c1) && al16(g0) && al16(g1);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)parts), block(256);
#define PST_GO(L, Gd) SFM_LAUNCH_LDS((pstoi_kernel<L, Gd>), grid, block, lds, st, e0, e1, c0, c1, band_w, g0, g1, ws, T, F, NB, FL, S, \
                                     clip, gscale, vec)
  if (layout == 0) {
    if (grad) PST_GO(0, true);
    else PST_GO(0, false);
  } else {
    if (grad) PST_GO(1, true);
    else PST_GO(1, false);
  }
#undef PST_GO
  const int rc = sfm_fold_partials_f64(ws, ws + parts, 1, 1, 1, (int)parts, 0, stream);
  if (rc != SFM_OK) return rc;
  SFM_LAUNCH(scaled_sum_kernel, dim3(1), dim3(64), 0, st, ws + parts, -1.0 / count, loss);
  return SFM_OK;
}

// loss[0] = mean (pred - target)^2 over n elements; grad (or NULL) = 2 (pred - target) / n.  ws: sfm_mse_loss_ws_doubles doubles
// of scratch (one partial per workgroup, then their sum; sized for the cap, whatever n).
static constexpr int MSE_MAX_BLOCKS = 1024;
extern "C" long long sfm_mse_loss_ws_doubles(long long n) { (void)n; return MSE_MAX_BLOCKS + 1; }
extern "C" int sfm_mse_loss(const float* pred, const float* target, float* loss, float* grad, double* ws, long long n,
                            void* stream) {
  if (!pred || !target || !loss || !ws) return SFM_ERR_ARG;
  if (n <= 0) return SFM_ERR_SHAPE;
  const long long nb = sfm_capped_blocks(n, 1024, MSE_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  SFM_LAUNCH(mse_kernel, dim3((unsigned)nb), dim3(256), 0, st, pred, target, grad, ws, n, 2.0 / (double)n);
  const int rc = sfm_fold_partials_f64(ws, ws + nb, 1, 1, 1, (int)nb, 0, stream);
  if (rc != SFM_OK) return rc;
  SFM_LAUNCH(scaled_sum_kernel, dim3(1), dim3(64), 0, st, ws + nb, 1.0 / (double)n, loss);
  return SFM_OK;
}
