// SpeechEnhancementDNN (models/dnn.py of the reference): one Linear + activation (+ dropout) per launch, and the activation's
// backward.
//
// dnn_layer_kernel: out[M, N] = act(A[M, K] W[N, Kpad]^T + bias) on v_mfma_f32_32x32x16_{f16,bf16}, fp32 accumulation.
//   Tile 128 rows x BN columns (BN = 128, or 64 when N <= 64: the output layer launches no idle column tile), BK = 64, 4 waves
//   as 2 x 2, wave tile 64 x BN / 2.  Both operands are staged through registers, because the A operand is not a copy: it is
//   converted from fp32 (rows32) or gathered from 2 ctx + 1 neighbouring raw rows, normalised, clipped and converted (context)
//   on the way, so that the [M, K] 16-bit (or, for the context, fp32) operand never exists in memory.  One LDS buffer, the
//   loads of k-tile t + 1 are issued after the barrier that publishes tile t and land under its MFMAs; LDS rows are 128 B with
//   the 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7): conflict-free ds_read_b128 fragment reads (as gemm16v2.hip).
//   The context mode reads pairs (D even, >= 8: a chunk of 8 columns lies in at most two neighbouring frames) and multiplies by 1 / std
//   kept in LDS beside the mean.  rows32 reads with 8-byte loads when the rows are 8-byte aligned (K = 594: 2376 B) and with 4-byte loads otherwise, never
//   wider, and never past column K of a row.  The k order of an output element is fixed: the same bits from run to run, and for
//   a row alone or inside any M.
//   Epilogue: bias, ReLU or sigmoid, dropout keep(seed, m N + n) after the ReLU (sfm_keep_scale: the hash and the element index of
//   every other dropout of the library); 16-bit rows with the pad columns N .. ldo written as zeros (the next layer's K padding),
//   or fp32 rows.
// dnn_act_bwd_kernel: dz = dy * act'(.) from the saved OUTPUT of the layer (ReLU + dropout: positive exactly where the unit was
//   active and kept; sigmoid: y (1 - y)), written as the zero-padded 16-bit rows the weight- and data-gradient GEMMs read.
#include "sfm_common.h"

static_assert(SFM_DNN_ROW_TILE == 128, "rows of a workgroup: four 32-row MFMA tiles, staged as one 128-row operand tile");
#define DNN_TILE_BYTES (SFM_DNN_ROW_TILE * 128)        // one operand tile: 128 rows x 64 16-bit elements

struct DnnParams {
  const void* A;          // rows16: 16-bit [M, lda]; rows32: fp32 [M, lda]; context: raw fp32 [B, T, D]
  const int* frames;      // context: int32 [B] live frames per utterance, or NULL (= T)
  const float* mean;      // context: [K] or NULL
  const float* stdv;
  const u16* W;           // [Npad, Kpad]
  const float* bias;      // [Npad] or NULL
  void* out;
  long long lda, ldo;
  int M, N, K, T, D, ctx, Kpad, Npad, out_f32, act, pair;
  float p_drop, inv_keep;
  uint32_t seed;
  // indexed context (sfm_dnn_layer_indexed): A = raw [n_frames, D] packed, T = n_frames
  const int* index;       // int32 [M]: the packed frame of row m (< 0 or >= n_frames: a zero row)
  const int* bounds;      // int32 [n_frames, 2]: first and one-past-last packed row of the frame's utterance
  u16* a16;               // [M, ld16] or NULL: the staged 16-bit operand rows, written by the workgroups of column tile 0
  long long ld16;
};

enum { DNN_ROWS16 = 0, DNN_ROWS32 = 1, DNN_CONTEXT = 2, DNN_INDEXED = 3 };

template <class T, int AMODE, int BN>
__global__ __launch_bounds__(256) void dnn_layer_kernel(DnnParams p) {
  constexpr int WN = BN / 2, NJ = WN / 32, NW = BN / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_mean = reinterpret_cast<float*>(smem + 2 * DNN_TILE_BYTES);   // context with statistics: [nt * 64], then 1 / std
  const int nt = (p.K + 63) >> 6;
  float* s_rstd = s_mean + nt * 64;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hl = lane >> 5;
  const int nNt = (p.N + BN - 1) / BN;
  const int ntile = blockIdx.x % nNt, mtile = blockIdx.x / nNt;
  const int n0 = ntile * BN, m0 = mtile * SFM_DNN_ROW_TILE;
  const int c8 = tid & 7, r0 = tid >> 3;                     // this thread stages chunk c8 of rows r0, r0 + 32, r0 + 64, r0 + 96
  const bool has_stats = (AMODE == DNN_CONTEXT || AMODE == DNN_INDEXED) && p.mean != nullptr;

  if (has_stats) {
    for (int k = tid; k < nt * 64; k += 256) {
      s_mean[k] = k < p.K ? p.mean[k] : 0.f;
      s_rstd[k] = k < p.K ? 1.0f / p.stdv[k] : 1.f;
    }
  }

  // context: the utterance, the frame and the live frame count of each of the thread's four rows (src == NULL: a zero row)
  const float* src[4];
  int frame_n[4], frame_tb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    src[i] = nullptr;
    frame_n[i] = frame_tb[i] = 0;
    const int row = m0 + r0 + 32 * i;
    if (AMODE == DNN_CONTEXT && row < p.M) {
      const int b = row / p.T, n = row - b * p.T;
      int tb = p.frames ? p.frames[b] : p.T;
      tb = tb < 0 ? 0 : (tb > p.T ? p.T : tb);
      if (n < tb) {
        src[i] = reinterpret_cast<const float*>(p.A) + (long long)b * p.T * p.D;
        frame_n[i] = n;
        frame_tb[i] = tb;
      }
    }
    if constexpr (AMODE == DNN_INDEXED) {
      // the row's packed frame and its utterance's bounds: an index load and one 8-byte load per row, once, ahead of the k loop;
      // from here on the row is an utterance (src), a frame in it and its frame count, as in the context mode
      if (row < p.M) {
        const int f = p.index[row];
        if (f >= 0 && f < p.T) {
          const int2 lh = *reinterpret_cast<const int2*>(p.bounds + 2 * (long long)f);
          const int lo = lh.x < 0 ? 0 : lh.x, hi = lh.y > p.T ? p.T : lh.y;
          if (lo <= f && f < hi) {
            src[i] = reinterpret_cast<const float*>(p.A) + (long long)lo * p.D;
            frame_n[i] = f - lo;
            frame_tb[i] = hi - lo;
          }
        }
      }
    }
  }

  u32x4 raw16[4];
  float raw32[4][8];
  u32x4 wraw[NW];

  auto fetch = [&](int kt) {
    const int k0 = kt * 64 + c8 * 8;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int n = n0 + r0 + 32 * i;
      wraw[i] = u32x4{0u, 0u, 0u, 0u};
      if (n < p.Npad) wraw[i] = *reinterpret_cast<const u32x4*>(p.W + (long long)n * p.Kpad + k0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + r0 + 32 * i;
      if constexpr (AMODE == DNN_ROWS16) {
        raw16[i] = u32x4{0u, 0u, 0u, 0u};
        if (row < p.M && k0 < p.K)                            // the rows are zero padded to a multiple of 8 columns
          raw16[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const u16*>(p.A) + (long long)row * p.lda + k0);
      } else if constexpr (AMODE == DNN_ROWS32) {
        const float* a = reinterpret_cast<const float*>(p.A) + (long long)row * p.lda + k0;
        if (row < p.M && k0 + 8 <= p.K && p.pair) {
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            const float2 v = *reinterpret_cast<const float2*>(a + e);
            raw32[i][e] = v.x;
            raw32[i][e + 1] = v.y;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) raw32[i][e] = (row < p.M && k0 + e < p.K) ? a[e] : 0.f;
        }
      } else {
        // D is even and >= 8: the chunk's 8 columns lie in at most two neighbouring frames of the context, pairs never straddle them
#pragma unroll
        for (int e = 0; e < 8; ++e) raw32[i][e] = 0.f;
        if (src[i] != nullptr && k0 < p.K) {
          const int j0 = k0 / p.D, c0 = k0 - j0 * p.D;
          int s0 = frame_n[i] - p.ctx + j0, s1 = s0 + 1;
          const int last = frame_tb[i] - 1;
          s0 = s0 < 0 ? 0 : (s0 > last ? last : s0);
          s1 = s1 < 0 ? 0 : (s1 > last ? last : s1);
          const float* q0 = src[i] + (long long)s0 * p.D + c0;
          const float* q1 = src[i] + (long long)s1 * p.D + (c0 - p.D);
#pragma unroll
          for (int e = 0; e < 8; e += 2) {
            if (k0 + e < p.K) {                               // K is even: the pair is whole
              const float2 v = *reinterpret_cast<const float2*>((c0 + e < p.D ? q0 : q1) + e);
              raw32[i][e] = v.x;
              raw32[i][e + 1] = v.y;
            }
          }
        }
      }
    }
  };

  unsigned char* sA = smem;
  unsigned char* sB = smem + DNN_TILE_BYTES;

  auto stage = [&](int kt) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int row = r0 + 32 * i;
      *reinterpret_cast<u32x4*>(sB + row * 128 + ((c8 ^ ((row >> 1) & 7)) << 4)) = wraw[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r0 + 32 * i;
      u32x4 v;
      if constexpr (AMODE == DNN_ROWS16) {
        v = raw16[i];
      } else {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = raw32[i][e];
        if (has_stats && src[i] != nullptr) {
          const int k0 = kt * 64 + c8 * 8;
          float mu[8], rs[8];
          *reinterpret_cast<f32x4*>(mu) = *reinterpret_cast<const f32x4*>(s_mean + k0);
          *reinterpret_cast<f32x4*>(mu + 4) = *reinterpret_cast<const f32x4*>(s_mean + k0 + 4);
          *reinterpret_cast<f32x4*>(rs) = *reinterpret_cast<const f32x4*>(s_rstd + k0);
          *reinterpret_cast<f32x4*>(rs + 4) = *reinterpret_cast<const f32x4*>(s_rstd + k0 + 4);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float x = isfinite(f[e]) ? f[e] : 0.f;
            x = (x - mu[e]) * rs[e];
            f[e] = x < -10.f ? -10.f : (x > 10.f ? 10.f : x);           // np.clip: a nan stays a nan
          }
        }
        v = u32x4{pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7])};
      }
      *reinterpret_cast<u32x4*>(sA + row * 128 + ((c8 ^ ((row >> 1) & 7)) << 4)) = v;
      if constexpr (AMODE == DNN_INDEXED) {
        // the first layer's weight gradient reads these rows (ld16 = 64 nt: every chunk of every k tile lies inside the row;
        // the columns K .. ld16 were staged as zeros)
        if (p.a16 != nullptr && ntile == 0 && m0 + row < p.M)
          *reinterpret_cast<u32x4*>(p.a16 + (long long)(m0 + row) * p.ld16 + kt * 64 + c8 * 8) = v;
      }
    }
  };

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int fa_off[2][4], fb_off[NJ][4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wm * 64 + i * 32 + l31;
#pragma unroll
    for (int s = 0; s < 4; ++s) fa_off[i][s] = row * 128 + (((2 * s + hl) ^ ((row >> 1) & 7)) << 4);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int row = wn * WN + j * 32 + l31;
#pragma unroll
    for (int s = 0; s < 4; ++s) fb_off[j][s] = row * 128 + (((2 * s + hl) ^ ((row >> 1) & 7)) << 4);
  }

  auto compute = [&]() {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 fa[2], fb[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const u32x4*>(sA + fa_off[i][s]);
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[j] = *reinterpret_cast<const u32x4*>(sB + fb_off[j][s]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = T::mfma(fa[i], fb[j], acc[i][j]);
    }
  };

  fetch(0);
  for (int t = 0; t < nt; ++t) {
    __syncthreads();                                          // the MFMAs of tile t - 1 have read the buffer (t = 0: the statistics are in LDS)
    stage(t);
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);
    compute();
  }

  // ---- epilogue: lanes 0..31 of a register hold 32 consecutive columns of one row ----
  u16* o16 = reinterpret_cast<u16*>(p.out);
  float* o32 = reinterpret_cast<float*>(p.out);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = n0 + wn * WN + j * 32 + l31;
    const float bias = (p.bias != nullptr && col < p.N) ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + i * 32 + mfma_row(r, lane);
        if (row >= p.M) continue;
        if (col < p.N) {
          float v = acc[i][j][r] + bias;
          if (p.act == SFM_DNN_ACT_RELU) {
            v = v > 0.f ? v : 0.f;
            if (p.p_drop > 0.f) v *= sfm_keep_scale(p.seed, (unsigned long long)row * p.N + col, p.p_drop, p.inv_keep);
          } else if (p.act == SFM_DNN_ACT_SIGMOID) {
            v = sigmoid_f(v);
          }
          if (p.out_f32) o32[(long long)row * p.ldo + col] = v;
          else o16[(long long)row * p.ldo + col] = T::from_f32(v);
        } else if (!p.out_f32 && col < p.ldo) {
          o16[(long long)row * p.ldo + col] = 0;
        }
      }
    }
  }
  // pad columns beyond the last column tile (a row stride wider than the tiles cover)
  const int covered = nNt * BN;
  if (!p.out_f32 && ntile == nNt - 1 && p.ldo > covered) {
    const int extra = (int)(p.ldo - covered);
    const int rows = p.M - m0 < SFM_DNN_ROW_TILE ? p.M - m0 : SFM_DNN_ROW_TILE;
    for (int idx = tid; idx < rows * extra; idx += 256) {
      const int r = idx / extra, c = idx - r * extra;
      o16[(long long)(m0 + r) * p.ldo + covered + c] = 0;
    }
  }
}

template <class T, int AMODE>
static int dnn_layer_launch(const DnnParams& p, int lds, hipStream_t stream) {
  const int nMt = (p.M + SFM_DNN_ROW_TILE - 1) / SFM_DNN_ROW_TILE;
  if (p.N <= 64) {
    SFM_LAUNCH((dnn_layer_kernel<T, AMODE, 64>), dim3((unsigned)nMt), dim3(256), lds, stream, p);
  } else {
    const long long blocks = (long long)nMt * ((p.N + 127) / 128);
    if (blocks > 0x7fffffffLL) return SFM_ERR_SHAPE;
    SFM_LAUNCH((dnn_layer_kernel<T, AMODE, 128>), dim3((unsigned)blocks), dim3(256), lds, stream, p);
  }
  return SFM_OK;
}

template <class T>
static int dnn_layer_mode(const DnnParams& p, int a_mode, int lds, hipStream_t stream) {
  if (a_mode == DNN_ROWS16) return dnn_layer_launch<T, DNN_ROWS16>(p, lds, stream);
  if (a_mode == DNN_ROWS32) return dnn_layer_launch<T, DNN_ROWS32>(p, lds, stream);
  return dnn_layer_launch<T, DNN_CONTEXT>(p, lds, stream);
}

extern "C" int sfm_dnn_layer(const void* A, const int* frames, const float* mean, const float* stdv, const void* W,
                             const float* bias, void* out, int a_mode, int M, int N, int K, long long lda, int T, int D, int ctx,
                             int Kpad, int Npad, long long ldo, int out_f32, int act, float p_drop, unsigned int seed, int dtype,
                             void* stream) {
  if (!A || !W || !out || (mean == nullptr) != (stdv == nullptr)) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  if (a_mode < DNN_ROWS16 || a_mode > DNN_CONTEXT || act < SFM_DNN_ACT_NONE || act > SFM_DNN_ACT_SIGMOID ||
      (out_f32 != 0 && out_f32 != 1))
    return SFM_ERR_ARG;
  if (!(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && act != SFM_DNN_ACT_RELU)) return SFM_ERR_ARG;
  if (a_mode != DNN_CONTEXT && (frames || mean)) return SFM_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || Kpad < K || (Kpad % 64) != 0 || Npad < N || (Npad % 64) != 0 || ldo < N) return SFM_ERR_SHAPE;
  if ((long long)M * N > 0x7fffffffffLL || K > (1 << 24)) return SFM_ERR_SHAPE;
  if ((((uintptr_t)W) % 16) != 0) return SFM_ERR_ARG;
  int lds = 2 * DNN_TILE_BYTES;
  DnnParams p;
  p.pair = 0;
  if (a_mode == DNN_ROWS16) {
    if (lda < (K + 7) / 8 * 8 || (lda % 8) != 0) return SFM_ERR_SHAPE;
    if ((((uintptr_t)A) % 16) != 0) return SFM_ERR_ARG;
  } else if (a_mode == DNN_ROWS32) {
    if (lda < K) return SFM_ERR_SHAPE;
    if ((((uintptr_t)A) % 4) != 0) return SFM_ERR_ARG;
    p.pair = ((((uintptr_t)A) % 8) == 0 && (lda % 2) == 0) ? 1 : 0;
  } else {
    if (T <= 0 || D < 8 || (D % 2) != 0 || ctx < 0 || ctx > 64 || (M % T) != 0 || (long long)D * (2 * ctx + 1) != K) return SFM_ERR_SHAPE;
    if ((((uintptr_t)A) % 8) != 0) return SFM_ERR_ARG;
    if (mean) {
      if (K > SFM_DNN_CONTEXT_MAX_K) return SFM_ERR_SHAPE;                     // the statistics sit in LDS beside the tiles: 64 KB in all
      lds += 2 * ((K + 63) / 64 * 64) * (int)sizeof(float);
    }
  }
  p.A = A; p.frames = frames; p.mean = mean; p.stdv = stdv; p.W = (const u16*)W; p.bias = bias; p.out = out;
  p.lda = lda; p.ldo = ldo; p.M = M; p.N = N; p.K = K; p.T = T; p.D = D; p.ctx = ctx; p.Kpad = Kpad; p.Npad = Npad;
  p.out_f32 = out_f32; p.act = act; p.p_drop = p_drop; p.inv_keep = 1.0f / (1.0f - p_drop); p.seed = seed;
  p.index = nullptr; p.bounds = nullptr; p.a16 = nullptr; p.ld16 = 0;
  if (dtype == SFM_DT_F16) return dnn_layer_mode<F16>(p, a_mode, lds, (hipStream_t)stream);
  return dnn_layer_mode<BF16>(p, a_mode, lds, (hipStream_t)stream);
}

// The first layer on an index list: the context mode with a per-row frame in place of (row / T, row % T)
extern "C" int sfm_dnn_layer_indexed(const float* raw, const int* bounds, const int* index, const float* mean, const float* stdv,
                                     const void* W, const float* bias, void* out, void* a16_out, int M, int N, int K, int n_frames,
                                     int D, int ctx, int Kpad, int Npad, long long ldo, long long ld16, int out_f32, int act,
                                     float p_drop, unsigned int seed, int dtype, void* stream) {
  if (!raw || !bounds || !index || !W || !out || (mean == nullptr) != (stdv == nullptr)) return SFM_ERR_ARG;
  if (act < SFM_DNN_ACT_NONE || act > SFM_DNN_ACT_SIGMOID || (out_f32 != 0 && out_f32 != 1)) return SFM_ERR_ARG;
  if (!(p_drop >= 0.f && p_drop < 1.f) || (p_drop > 0.f && act != SFM_DNN_ACT_RELU)) return SFM_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0 || Kpad < K || (Kpad % 64) != 0 || Npad < N || (Npad % 64) != 0 || ldo < N) return SFM_ERR_SHAPE;
  if ((long long)M * N > 0x7fffffffffLL || K > (1 << 24)) return SFM_ERR_SHAPE;
  if (n_frames <= 0 || D < 8 || (D % 2) != 0 || ctx < 0 || ctx > 64 || (long long)D * (2 * ctx + 1) != K) return SFM_ERR_SHAPE;
  if (a16_out && ld16 != (long long)((K + 63) / 64) * 64) return SFM_ERR_SHAPE;
  if ((((uintptr_t)W) % 16) != 0 || (((uintptr_t)raw) % 8) != 0 || (((uintptr_t)bounds) % 8) != 0 || (((uintptr_t)a16_out) % 16) != 0)
    return SFM_ERR_ARG;
  int lds = 2 * DNN_TILE_BYTES;
  if (mean) {
    if (K > SFM_DNN_CONTEXT_MAX_K) return SFM_ERR_SHAPE;
    lds += 2 * ((K + 63) / 64 * 64) * (int)sizeof(float);
  }
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;      // last: a call refused for it alone passed every other check
  DnnParams p;
  p.A = raw; p.frames = nullptr; p.mean = mean; p.stdv = stdv; p.W = (const u16*)W; p.bias = bias; p.out = out;
  p.lda = 0; p.ldo = ldo; p.M = M; p.N = N; p.K = K; p.T = n_frames; p.D = D; p.ctx = ctx; p.Kpad = Kpad; p.Npad = Npad;
  p.out_f32 = out_f32; p.act = act; p.pair = 0; p.p_drop = p_drop; p.inv_keep = 1.0f / (1.0f - p_drop); p.seed = seed;
  p.index = index; p.bounds = bounds; p.a16 = (u16*)a16_out; p.ld16 = ld16;
  if (dtype == SFM_DT_F16) return dnn_layer_launch<F16, DNN_INDEXED>(p, lds, (hipStream_t)stream);
  return dnn_layer_launch<BF16, DNN_INDEXED>(p, lds, (hipStream_t)stream);
}

// one thread per 8 consecutive columns of a dz row: [M, ldz / 8] chunks; columns N .. ldz are written as zeros
template <class T>
__global__ __launch_bounds__(256) void dnn_act_bwd_kernel(const void* __restrict__ dy, int dy_f32, long long ldy,
                                                          const void* __restrict__ saved, long long ld_saved, u16* __restrict__ dz,
                                                          long long ldz, int M, int N, int act, float inv_keep) {
  const long long chunks = ldz >> 3;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)M * chunks) return;
  const long long row = idx / chunks;
  const int c0 = (int)(idx - row * chunks) * 8;
  float g[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = c0 + e;
    float v = 0.f;
    if (c < N) {
      v = dy_f32 ? reinterpret_cast<const float*>(dy)[row * ldy + c] : T::to_f32(reinterpret_cast<const u16*>(dy)[row * ldy + c]);
      if (act == SFM_DNN_ACT_RELU) {
        const float h = T::to_f32(reinterpret_cast<const u16*>(saved)[row * ld_saved + c]);
        v = h > 0.f ? v * inv_keep : 0.f;
      } else if (act == SFM_DNN_ACT_SIGMOID) {
        const float y = reinterpret_cast<const float*>(saved)[row * ld_saved + c];
        v = v * y * (1.f - y);
      }
    }
    g[e] = v;
  }
  *reinterpret_cast<u32x4*>(dz + row * ldz + c0) =
      u32x4{pack2<T>(g[0], g[1]), pack2<T>(g[2], g[3]), pack2<T>(g[4], g[5]), pack2<T>(g[6], g[7])};
}

extern "C" int sfm_dnn_act_bwd(const void* dy, int dy_f32, long long ldy, const void* saved, long long ld_saved, void* dz,
                               long long ldz, int M, int N, int act, float p_drop, int dtype, void* stream) {
  if (!dy || !dz || (act != SFM_DNN_ACT_NONE && !saved)) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  if (act < SFM_DNN_ACT_NONE || act > SFM_DNN_ACT_SIGMOID || (dy_f32 != 0 && dy_f32 != 1) || !(p_drop >= 0.f && p_drop < 1.f) ||
      (p_drop > 0.f && act != SFM_DNN_ACT_RELU))
    return SFM_ERR_ARG;
  if (M <= 0 || N <= 0 || ldy < N || (act != SFM_DNN_ACT_NONE && ld_saved < N) || ldz < N || (ldz % 8) != 0) return SFM_ERR_SHAPE;
  if ((((uintptr_t)dz) % 16) != 0) return SFM_ERR_ARG;
  const long long work = (long long)M * (ldz >> 3);
  const long long blocks = (work + 255) / 256;
  if (blocks > 0x7fffffffLL) return SFM_ERR_SHAPE;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((dnn_act_bwd_kernel<F16>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, ldy, saved, ld_saved,
               (u16*)dz, ldz, M, N, act, inv_keep);
  else
    SFM_LAUNCH((dnn_act_bwd_kernel<BF16>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, ldy, saved, ld_saved,
               (u16*)dz, ldz, M, N, act, inv_keep);
  return SFM_OK;
}

// ---- the training loss on gathered targets, and the output layer's pre-activation cotangent, in one pass over y ----------------
// mse_gather_kernel: one thread per 8 consecutive columns of a dz row (as dnn_act_bwd_kernel), grid-stride over the [M, ldz / 8]
//   chunks; t = clip(nan_to_num(mask[index[m], c], nan 0, +inf 1, -inf 0), 0, 1) (the Dataset's treatment of the mask),
//   d = y - t, the squares summed in fp64 per workgroup -> ws[workgroup]; dz = (S 2 / (M C)) d y (1 - y) in fp32, rounded once.
// mse_gather_finish_kernel: one workgroup folds the partials in workgroup order, loss = sum / (M C), and keeps the epoch's record
//   rec = {sum of finite batch losses, finite batches, non-finite batches, the last loss}; a non-finite loss raises ctl[2], the
//   optimiser's skip flag.
static_assert(SFM_MSE_GATHER_MAX_BLOCKS == 1024, "one fp64 partial per workgroup: the scratch the wrapper allocates");

__device__ __forceinline__ float mask_target(float t) {
  if (t != t) return 0.f;
  return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);                 // -inf -> 0, +inf -> 1
}

template <class T>
__global__ __launch_bounds__(256) void mse_gather_kernel(const float* __restrict__ y, const float* __restrict__ mask,
                                                         const int* __restrict__ index, const float* __restrict__ loss_scale,
                                                         u16* __restrict__ dz, long long ldz, double* __restrict__ ws, int M, int C,
                                                         int n_frames) {
  __shared__ double red[4];
  const long long chunks = ldz >> 3;
  const long long work = (long long)M * chunks;
  const float S = loss_scale ? loss_scale[0] : 1.f;
  const float k = (float)((double)S * 2.0 / ((double)M * (double)C));
  double sq = 0.0;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < work; idx += (long long)gridDim.x * 256) {
    const long long row = idx / chunks;
    const int c0 = (int)(idx - row * chunks) * 8;
    const int f = index[row];
    const bool live = f >= 0 && f < n_frames;
    float g[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      g[e] = 0.f;
      if (live && c < C) {
        const float yv = y[row * C + c];
        const float d = yv - mask_target(mask[(long long)f * C + c]);
        sq += (double)d * (double)d;
        g[e] = k * d * (yv * (1.f - yv));
      }
    }
    if (dz != nullptr)
      *reinterpret_cast<u32x4*>(dz + row * ldz + c0) =
          u32x4{pack2<T>(g[0], g[1]), pack2<T>(g[2], g[3]), pack2<T>(g[4], g[5]), pack2<T>(g[6], g[7])};
  }
  sq = wave_sum_d(sq);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void mse_gather_finish_kernel(const double* __restrict__ ws, int nb, double count,
                                                                float* __restrict__ loss, double* __restrict__ rec,
                                                                double* __restrict__ ctl) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += ws[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < 256; ++i) total += part[i];
  const double l = total / count;
  const bool finite = l == l && l <= 1.7e308 && l >= -1.7e308;
  if (loss) loss[0] = (float)l;
  if (rec) {
    if (finite) { rec[0] += l; rec[1] += 1.0; } else { rec[2] += 1.0; }
    rec[3] = l;
  }
  if (ctl && !finite) ctl[2] = 1.0;
}

extern "C" int sfm_mse_gather_loss(const float* y, const float* mask, const int* index, const float* loss_scale, void* dz, long long ldz,
                                   float* loss, double* rec, double* ctl, double* ws, int M, int C, int n_frames, int dtype,
                                   void* stream) {
  if (!y || !mask || !index || !ws || (!loss && !rec)) return SFM_ERR_ARG;
  if (M <= 0 || C <= 0 || n_frames <= 0 || ldz < C || (ldz % 8) != 0) return SFM_ERR_SHAPE;
  if ((((uintptr_t)dz) % 16) != 0) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;      // last, as in sfm_dnn_layer_indexed
  const long long work = (long long)M * (ldz >> 3);
  const int nb = (int)sfm_capped_blocks(work, 256, SFM_MSE_GATHER_MAX_BLOCKS);
  if (dtype == SFM_DT_F16)
    SFM_LAUNCH((mse_gather_kernel<F16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, y, mask, index, loss_scale, (u16*)dz, ldz,
               ws, M, C, n_frames);
  else
    SFM_LAUNCH((mse_gather_kernel<BF16>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, y, mask, index, loss_scale, (u16*)dz, ldz,
               ws, M, C, n_frames);
  SFM_LAUNCH(mse_gather_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, nb, (double)M * (double)C, loss, rec,
             ctl);
  return SFM_OK;
}
