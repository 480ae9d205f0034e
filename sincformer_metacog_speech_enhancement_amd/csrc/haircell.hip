// Meddis inner hair cell (signal_processing/haircell.py): per (utterance, channel) one chain of L Euler steps in fp64,
//   s = max(x[t] + A, 0), k = s / (s + B),
//   q = max(q + dt (y (M - q) + xr w - k q), 0), c = max(c + dt (k q - l c - r c), 0), w = max(w + dt (r c - xr w), 0), out[t] = h c
// with the reference's operation order and its three clamps (max(v, 0) keeps v unless 0 > v, as Python's max does).  Compiled
// with -ffp-contract=off: every operation is one IEEE double operation, so a chain equals the reference's loop bit for bit.
//
// Layout: a lane owns a chain, and a lane that walked its own row of x [N, L] would read 64 rows 4 L bytes apart per step.  A
// wave therefore stages tiles of 64 chains x 64 samples through LDS: row by row, the 64 lanes read 64 consecutive samples (256
// contiguous bytes), form k - which depends on the input alone, so the division leaves the recurrence - and park it as a double
// at kt[row][t], rows 65 doubles apart (lane stride 130 dwords: ds_read_b64 over 32 lanes touches each bank pair once).  Then
// each lane steps through its row.  The firing rate goes back into the slot it read and leaves row by row, 512 contiguous bytes
// per store (sfm_haircell), or is only summed (sfm_haircell_frames): the chain carries the sums of the at most two frames that
// cover its sample (frame <= 2 hop) and writes a frame's mean when its last sample has passed; the rate signal never exists.
// One wave per workgroup; no atomics; a chain gets the bits it gets alone.
#include "sfm_common.h"

#define HC_T 64                       // samples per tile
#define HC_LD 65                      // row stride of the tile (doubles)
enum { HC_A, HC_B, HC_Y, HC_L, HC_R, HC_X, HC_H, HC_M, HC_DT, HC_Q0, HC_C0, HC_W0, HC_NPAR };
static_assert(HC_NPAR == SFM_HC_PARAMS, "the doubles of `par`");

__device__ __forceinline__ double hc_clamp(double v) { return (0.0 > v) ? 0.0 : v; }

// x [N, L] fp32, chain = b * C + ch; par [HC_NPAR] fp64.  FRAMES = 0: out [N, L] fp64.  FRAMES = 1: out [N, T] fp64 = frame means,
// 0 from T_b on.  grid (ceil(N / 64)), block 64.
template <int FRAMES>
__global__ __launch_bounds__(64) void haircell_kernel(const float* __restrict__ x, const double* __restrict__ par,
                                                      const int* __restrict__ lengths, double* __restrict__ out, int N, int C, int L,
                                                      int frame, int hop, int T) {
  __shared__ double kt[64 * HC_LD];
  const int lane = threadIdx.x, ch0 = blockIdx.x * 64, chain = ch0 + lane;
  const bool mine = chain < N;
  const double A = par[HC_A], Bp = par[HC_B], y = par[HC_Y], l = par[HC_L], r = par[HC_R], xr = par[HC_X], h = par[HC_H],
               M = par[HC_M], dt = par[HC_DT];
  double q = par[HC_Q0], c = par[HC_C0], w = par[HC_W0];
  int Lb = L;
  if (mine && lengths) {
    Lb = lengths[chain / C];
    Lb = Lb < 0 ? 0 : (Lb > L ? L : Lb);
  }
  const int Tb = FRAMES ? ((Lb >= frame) ? (Lb - frame) / hop + 1 : 0) : 0;
  int n0 = 0, off = 0, done = 0;                               // FRAMES: hop-block of t, t - n0 hop, frames written
  double s0 = 0.0, s1 = 0.0;                                   // sums of frame n0 and of frame n0 - 1
  const int rows = (N - ch0 < 64) ? N - ch0 : 64;
  for (int t0 = 0; t0 < L; t0 += HC_T) {
    const int nt = (L - t0 < HC_T) ? L - t0 : HC_T;
    if (lane < nt) {
      const float* xp = x + (long long)ch0 * L + t0 + lane;
#pragma unroll 8
      for (int row = 0; row < rows; ++row) {
        const double s = hc_clamp((double)xp[(long long)row * L] + A);
        kt[row * HC_LD + lane] = s / (s + Bp);
      }
    }
    __syncthreads();
    if (mine) {
      double* kp = kt + lane * HC_LD;
      const int ne = (Lb - t0 < nt) ? Lb - t0 : nt;            // FRAMES: a chain ends at its utterance's length
      for (int i = 0; i < (FRAMES ? ne : nt); ++i) {
        const double k = kp[i];
        const double dq = dt * (y * (M - q) + xr * w - k * q);
        q = hc_clamp(q + dq);
        const double dc = dt * (k * q - l * c - r * c);
        c = hc_clamp(c + dc);
        const double dw = dt * (r * c - xr * w);
        w = hc_clamp(w + dw);
        const double v = h * c;
        if (!FRAMES) {
          kp[i] = v;
        } else {
          if (off < frame) s0 += v;
          if (n0 > 0 && off + hop < frame) s1 += v;
          if (n0 > 0 && off + hop == frame - 1 && n0 - 1 < Tb) { out[(long long)chain * T + n0 - 1] = s1 / (double)frame; ++done; }
          if (off == frame - 1 && n0 < Tb) { out[(long long)chain * T + n0] = s0 / (double)frame; ++done; }
          if (++off == hop) { off = 0; ++n0; s1 = s0; s0 = 0.0; }
        }
      }
    }
    __syncthreads();
    if (!FRAMES && lane < nt) {
      double* op = out + (long long)ch0 * L + t0 + lane;
      for (int row = 0; row < rows; ++row) op[(long long)row * L] = kt[row * HC_LD + lane];
    }
    if (!FRAMES) __syncthreads();
  }
  if (FRAMES && mine)
    for (int n = done; n < T; ++n) out[(long long)chain * T + n] = 0.0;
}

static bool hc_ok(int N, int C, int L) { return N > 0 && C > 0 && N % C == 0 && L > 0; }

extern "C" int sfm_haircell(const float* x, const double* par, double* out, int N, int L, void* stream) {
  if (!x || !par || !out) return SFM_ERR_ARG;
  if (!hc_ok(N, 1, L)) return SFM_ERR_SHAPE;
  SFM_LAUNCH((haircell_kernel<0>), dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, par, (const int*)nullptr, out, N, 1, L, 0,
             0, 0);
  return SFM_OK;
}

extern "C" int sfm_haircell_frames(const float* x, const double* par, const int* lengths, double* frames, int N, int C, int L,
                                   int frame, int hop, int T, void* stream) {
  if (!x || !par || !frames) return SFM_ERR_ARG;
  if (!hc_ok(N, C, L) || frame < 1 || hop < 1 || frame > 2 * hop || L < frame || T != (L - frame) / hop + 1) return SFM_ERR_SHAPE;
  SFM_LAUNCH((haircell_kernel<1>), dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, x, par, lengths, frames, N, C, L, frame, hop,
             T);
  return SFM_OK;
}
