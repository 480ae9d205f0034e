#include "gemm16_epi.h"

// ---------------------------------------------------------------------------------------------------------------
// conv16p: the PerceptionAgent's Conv1d layers (agents/perception.py:192-206, 167-171) with the GroupNorm + GELU of their
// INPUT applied while the operand is staged, so the normalised activation never exists in HBM:
//     y[b, l, n] = bias[n] + sum_{t, c} x[b, l s - p + t, c] W[n, (t, c)],   x = GELU( sc1[b,c] r1 + sh1[b,c]  [+ sc2[b,c] r2 + sh2[b,c]] )
// r1 (r2) = the RAW output of the producing conv(s), sc / sh = the finalised GroupNorm scale / shift of that output
// (sfm_gn_finalize); the two-input form is the residual block's  GELU(GN(main) + GN(skip))  (agents/perception.py:129).
// What changes against sfm_gemm16's implicit GEMM:
//   * the input rows of a 128-row output tile ("patch": 127 s + k rows x 64 channels) are fetched ONCE, transformed in
//     registers and written back to LDS: scale / shift, then GELU - for fp16 operands (the default policy) a logistic fit of the
//     normal CDF on packed fp16 pairs (gelu_lg_h2p below, with its error figures), for bf16 operands the erf form by
//     Abramowitz-Stegun 7.1.26 in fp32 (|err| < 1.5e-7);
//     the k taps then read the same patch at shifted rows (stride 2: even / odd input rows live in two planes, so that the
//     rows of consecutive outputs stay consecutive in LDS and the usual chunk swizzle keeps ds_read_b128 conflict-free).
//     The implicit im2col of sfm_gemm16 re-reads every input row k / s times from L2 and cannot transform in flight
//     (LDS-DMA), which is why a separate gn_apply pass (read + write of every activation) used to sit between two convs;
//   * more than 64 input channels: 64-channel slabs, one patch at a time, accumulators kept across slabs;
//   * the 1x1 stride-2 skip conv of a residual block reads the centre tap of the same patch: SKIP adds its k-tiles and a
//     second accumulator / output (N = 128 layers); N = 256 runs as two 128-column passes over the same patch (NPASS);
//   * weights stream L2 -> LDS by LDS-DMA in 128 x 64 tiles through a 2-stage ring, one barrier per k-tile, as in gemm16w.
// LDS: patch 16.6-33.8 KB + ring 32 KB: two workgroups per CU, so one's staging (VALU) overlaps the other's MFMA loop.
// The accumulators start from the bias (convp_acc_init); the epilogue (convp_epilogue_impl) takes the GroupNorm partials of the
// raw output from them and stores 16-byte rows.
// ---------------------------------------------------------------------------------------------------------------
struct ConvPParams {
  Gemm2Params g;                                       // main conv: W [N][KS * Cin] tap-major, bias, out, gn_partial, ...
  Gemm2Params gs;                                      // skip conv (SKIP): W [N][Cin], bias, out, gn_partial
  const u16* x1; const float* sc1; const float* sh1;
  const u16* x2; const float* sc2; const float* sh2;
  int Lin, Cin, pad, nMt;
  long long x_batch_stride;
};

__device__ __forceinline__ float gelu_as(float z) {    // z Phi(z), erf by A&S 7.1.26 (the backward in gn_bwd.hip uses the same)
  const float ax = fabsf(z) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);     // 1 ulp: the result is rounded to 16 bits afterwards
  const float ex = __builtin_amdgcn_exp2f(-0.72134752044448170368f * z * z);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float erfa = 1.0f - poly * ex;
  return z * (0.5f + 0.5f * copysignf(erfa, z));
}

// GELU on TWO fp16 values per instruction (v_pk_fma_f16 is a real 2 x, unlike v_pk_fma_f32), used when the stage's operand format
// is fp16 (the default policy).  The result is rounded to fp16 anyway, so the form is chosen for fp16 arithmetic, not carried over
// from the fp32 one:
//     GELU(z) = max(z, 0) - |z| Phi(-|z|),   Phi(-a) = e / (1 + e),   e = 2^(-a q(a)),   q = c0 + c1 a + c2 a^2 + c3 a^3 + c4 a^4
// a logistic fit of the normal CDF.  e <= 1, so nothing overflows; the tail is  |z| e  with e accurate relative to itself down to
// the subnormals (the A&S erf form computed 1 - poly * ex there, whose fp16 rounding near 1 is 2.4e-4: 9 % of GELU(-3), and all of
// it below -4); the last operation is ONE fma, so a large z comes back exactly (e t |z| < half an ulp from z = 3.45 on, e = 0 from
// a q(a) > 25 on) and the negative side ends in a zero.  q grows without bound (c4 > 0): |z| up to 65504 needs no clamp, q = inf gives
// e = 0, and no product is 0 x inf (q >= c0).  10 packed / bit operations and the same four transcendentals per pair, against 13.
// Coefficients: least squares on log2(Phi(a) / Phi(-a)) / a over (0, 5.8], then the fp16 neighbours of each searched for the
// smallest maximum error, in fp16 ulps of the float64 erf GELU, of this very sequence of fp16 roundings over all 63 488 finite
// inputs, under the condition that every z >= 3.447 (from where on the float64 GELU rounds to z) comes back as z even with the
// exponential one fp16 ulp off either way: at z = 3.447 the exact result lies 5e-7 above a rounding boundary, so that condition is
// a matter of which side -a q(a) rounds to.  tests/test_gelu_fp16_host.py pins the coefficients and repeats the sweep.  Largest
// error 11.9 ulps (at z = -4.16) and 1.02e-3 absolute (at z = 2.09, half an ulp of the result), the same on the MI355X as in the
// emulation, against 2 043 ulps and 1.93e-3 of the A&S form in fp16 (profiles/r23/gelu_fp16_sweep.txt); in ulps it is also the
// smaller of the two on each of [-6, -4), [-4, -2), [-2, -1), [-1, 0), [0, 1), [1, 2), [2, 4) taken alone.
// z itself (scale / shift of the GroupNorm) is still formed in fp32 from the fp16 inputs: a packed x * a + d would cancel
// |mean / std| ulps.
typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
#define SFM_GELU_H_C0 2.333984375f
#define SFM_GELU_H_C1 (-0.08050537109375f)
#define SFM_GELU_H_C2 0.1683349609375f
#define SFM_GELU_H_C3 (-0.0183258056640625f)
#define SFM_GELU_H_C4 0.0007991790771484375f
// z pair already packed (the GroupNorm affine of the fp16 inputs formed by v_fma_mixlo / mixhi_f16: fp32 arithmetic, ONE rounding
// to fp16, no unpack / pack instructions)
__device__ __forceinline__ uint32_t gelu_lg_h2p(uint32_t zb) {
  const h2_t z = __builtin_bit_cast(h2_t, zb);
  const h2_t az = __builtin_bit_cast(h2_t, zb & 0x7fff7fffu);
  h2_t q = az * (_Float16)SFM_GELU_H_C4 + (_Float16)SFM_GELU_H_C3;
  q = q * az + (_Float16)SFM_GELU_H_C2;
  q = q * az + (_Float16)SFM_GELU_H_C1;
  q = q * az + (_Float16)SFM_GELU_H_C0;
  const h2_t e = __builtin_elementwise_exp2(-(q * az));
  const h2_t u = e + (_Float16)1.0f;
  h2_t t;
  t[0] = __builtin_amdgcn_rcph(u[0]);
  t[1] = __builtin_amdgcn_rcph(u[1]);
  const h2_t m = az * e;
  // max(z, 0) on the bit patterns as signed 16-bit integers (every negative half, -0 included, is a negative integer): the
  // floating-point maximum would first canonicalise z, a second instruction
  typedef short s2_t __attribute__((ext_vector_type(2)));
  const h2_t r = __builtin_bit_cast(h2_t, __builtin_elementwise_max(__builtin_bit_cast(s2_t, zb), (s2_t)(short)0));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(-m, t, r));
}

// Epilogue of one 64 x 64 wave tile.  The accumulators hold the TRANSPOSED tile (weights were the A operand of the MFMAs):
// lane (m = lane & 31, h = lane >> 5) of tile (n-block j, m-block i) holds, in register r, output row m, channel
// n = (r & 3) + 8 (r >> 2) + 4 h: four consecutive channels per register quad.  So
//   * the GroupNorm partial sums (per 8 / 16 / 32-channel group over the tile's 64 rows) are in-lane sums over register
//     quads followed by DPP reductions over the lanes: no LDS;
//   * the 16-bit result of a quad is one 8-byte LDS write into a row-major [64][64] 16-bit image (144-byte rows), ONE
//     write -> read round trip for the whole tile, then eight 16-byte coalesced row stores.
// (A first version passed 8 x 8-row fp32 strips through LDS like gemm16's epilogue: 8 round trips, 9 k cycles per tile - as much
// as staging the patch and the MFMA loop together.  gemm16_epilogue_strips itself is not used here: it carries every
// activation / residual / dropout mode of sfm_gemm16 inline, and two instances of it made instruction fetch the bound.)
// Round 4 (the two epilogues of a b0.c1 + skip tile were 2 000 instructions, a third of the tile's cycles): FULL = every row of the
// wave's 64 x 64 tile is inside the utterance (a wave-uniform choice made by the caller): no row predicates in the statistics;
// the 16-bit converts are hoisted behind ONE branch on the output format (a select per convert computed both formats and chose:
// 2 x 64 converts + 128 v_cndmask per tile); the row stores are buffer stores (32-bit offsets against a per-utterance descriptor
// whose range check drops the rows beyond Lout: no 64-bit address arithmetic, no exec-mask branches).
template <class T, bool FULL>
__device__ __forceinline__ void convp_epilogue_impl(const Gemm2Params& g, f32x16 (&acc)[2][2], unsigned char* img,
                                                    int lane, int b, int colb, int row_base) {
  constexpr int ROWB = 144;                            // image row: 64 x 16-bit + 16 bytes of padding (fp32 mode: two passes)
  const int l31 = lane & 31, hl = lane >> 5;
  // ---- statistics (the accumulators started from the bias: convp_acc_init) ----
  float ps[2][4], pq[2][4];                            // per (n-block j, 8-channel quad-pair g): sums over this lane's rows
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float s_ = 0.f, q_ = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool rowok = FULL || (row_base + i * 32 + l31 < g.Lout);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[i][j][4 * gq + e];
          if (FULL && i == 0 && e == 0) {              // the sums start from their first term (0 + v is not folded: -0)
            s_ = v;
            q_ = v * v;
          } else if (rowok) {
            s_ += v;
            q_ = __builtin_fmaf(v, v, q_);
          }
        }
      }
      ps[j][gq] = s_;
      pq[j][gq] = q_;
    }
  if (g.gn_partial) {
    // lanes = rows (and the two channel halves of a quad pair): the 16 per-lane sums (8 chunks of 8 channels x {sum, sum of
    // squares}) go through ONE transposing reduction; lane v < 16 then holds the tile total of (stat = v >> 3, j = (v >> 2) & 1,
    // gq = v & 3).  Groups wider than 8 channels add the neighbouring lanes' chunks (gq pairs: xor 1, quads: xor 2).
    const int cpg = g.gn_group >> 3;                   // 8-channel chunks per group: 1, 2 or 4
    const int gsh = 31 - __builtin_clz(g.gn_group);    // gn_group is 8, 16 or 32 (sfm_conv16p checks): shifts, not divisions
    const int ngroups = g.N >> gsh;
    float v16[16];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        v16[j * 4 + gq] = ps[j][gq];
        v16[8 + j * 4 + gq] = pq[j][gq];
      }
    float tot = wave_sum16_transpose(v16, lane);
    if (cpg >= 2) tot += dpp_perm<0xB1>(tot);
    if (cpg == 4) tot += dpp_perm<0x4E>(tot);
    const int gq_ = lane & 3, j_ = (lane >> 2) & 1, stat = (lane >> 3) & 1;
    if (lane < 16 && (gq_ & (cpg - 1)) == 0 && (row_base >> 6) < g.gn_slots) {
      // the partials are fewer than B Lout words, and B Lout N outputs fit the device's memory: a 32-bit index
      const int sl = (b * g.gn_slots + (row_base >> 6)) * ngroups + ((colb + j_ * 32 + 8 * gq_) >> gsh);
      g.gn_partial[sl * 2 + stat] = tot;
    }
  }
  // ---- store: 16-bit through one LDS image; fp32 (the latent heads' consumers) as two 32-row halves through the same image ----
  const int osz = g.out_f32 == 1 ? 4 : 2;
  // rows >= Lout fall outside the descriptor's range and are dropped by the hardware
  auto ors = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<unsigned char*>(g.out) + (long long)b * g.o_batch_stride * osz), 0,
                                               g.Lout * g.ldo * osz, 0x00020000);
  if (g.out_f32 != 1) {
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
#define CONVP_PACK_IMG(PK)                                                                                             \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                        \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                        \
  _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                                                                   \
    u32x2 w;                                                                                                           \
    w[0] = PK(acc[i][j][4 * gq + 0], acc[i][j][4 * gq + 1]);                                                           \
    w[1] = PK(acc[i][j][4 * gq + 2], acc[i][j][4 * gq + 3]);                                                           \
    *reinterpret_cast<u32x2*>(img + (i * 32 + l31) * ROWB + (j * 32 + 8 * gq + 4 * hl) * 2) = w;                       \
  }
    if ((g.out_f32 == 2) == (T::id == SFM_DT_BF16)) { CONVP_PACK_IMG(F16::pack) } else { CONVP_PACK_IMG(BF16::pack) }
#undef CONVP_PACK_IMG
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    u32x4 rv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = lane + 64 * k;
      rv[k] = *reinterpret_cast<const u32x4*>(img + (c >> 3) * ROWB + (c & 7) * 16);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = lane + 64 * k;
      const int row = c >> 3, ch = c & 7;
      __builtin_amdgcn_raw_buffer_store_b128(rv[k], ors, ((row_base + row) * g.ldo + colb + ch * 8) * 2, 0, 0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          *reinterpret_cast<f32x4*>(img + l31 * 272 + (j * 32 + 8 * gq + 4 * hl) * 4) =
              f32x4{acc[i][j][4 * gq + 0], acc[i][j][4 * gq + 1], acc[i][j][4 * gq + 2], acc[i][j][4 * gq + 3]};
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = lane + 64 * k;
        const int row = c >> 4, ch = c & 15;           // 32 rows x 16 chunks of 4 floats
        const u32x4 v = *reinterpret_cast<const u32x4*>(img + row * 272 + ch * 16);
        __builtin_amdgcn_raw_buffer_store_b128(v, ors, ((row_base + i * 32 + row) * g.ldo + colb + ch * 4) * 4, 0, 0);
      }
    }
  }
}

template <class T>
__device__ __forceinline__ void convp_epilogue(const Gemm2Params& g, f32x16 (&acc)[2][2], unsigned char* img,
                                               int lane, int b, int colb, int row_base) {
  if (row_base + 64 <= g.Lout) convp_epilogue_impl<T, true>(g, acc, img, lane, b, colb, row_base);       // wave-uniform
  else convp_epilogue_impl<T, false>(g, acc, img, lane, b, colb, row_base);
}

// The accumulators of one 64 x 64 wave tile start from the bias of their channels (the register -> channel map above) instead of
// adding it in the epilogue: 16 LDS reads straight into the accumulator registers replace 64 adds and 8 LDS reads per tile.
// bias_s = the LDS copy made at kernel start.  Called behind the first patch's barriers, just before the first MFMA: loaded at
// kernel start the accumulators would be live across the first patch's staging, which cost b0.c2 its third workgroup per CU
// (135 -> 213 VGPRs) and spilled in the k 7 + skip kernels.
__device__ __forceinline__ void convp_acc_init(const float* bias_s, f32x16 (&acc)[2][2], int hl) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_s + j * 32 + 8 * gq + 4 * hl);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][j][4 * gq + e] = bv[e];
      }
}

#define CONVP_VARLEN 0
#include "conv16p_kernel.h"                            // conv16p_kernel: the dense form
#undef CONVP_VARLEN
#define CONVP_VARLEN 1
#include "conv16p_kernel.h"                            // conv16p_varlen_kernel: a length per utterance from two tables
#undef CONVP_VARLEN

template <class T, int KS, int STRIDE, int NPASS, bool SKIP, bool TWO_IN>
static int launch_convp(const ConvPParams& p, hipStream_t stream, const int* lin_tab = nullptr, const int* lout_tab = nullptr) {
  constexpr int R = 127 * STRIDE + KS;
  constexpr int PLANES = (STRIDE == 2 && KS > 1) ? 2 : 1;
  constexpr int PR = (((STRIDE == 2) ? (R + 1) / 2 : R) + 7) / 8 * 8;
  constexpr int patch = PLANES * PR * 128;
  constexpr int lds = patch + ((TWO_IN && patch > 2 * 128 * 128) ? patch : 2 * 128 * 128) + 384 * 4;   // + the bias copy
  if (lin_tab) {
    // fp16 operands only: the bf16 twin of the k 7 + skip + two-input kernel spills SGPRs, as its dense one does, and the ragged
    // path refuses a bf16 front end on the host (functional.perception_forward)
    if constexpr (T::id == SFM_DT_F16)
      SFM_LAUNCH_LDS((conv16p_varlen_kernel<T, KS, STRIDE, NPASS, SKIP, TWO_IN>), dim3(p.nMt * p.g.B), dim3(256), lds, stream, p,
                     lin_tab, lout_tab);
    else return SFM_ERR_SHAPE;
  } else
    SFM_LAUNCH_LDS((conv16p_kernel<T, KS, STRIDE, NPASS, SKIP, TWO_IN>), dim3(p.nMt * p.g.B), dim3(256), lds, stream, p);
  return SFM_OK;
}

static void convp_fill(Gemm2Params& g, const void* W, const float* bias, void* out, float* gn_partial, int B, int Lout, int N,
                       int Kpad, int out_f32, int gn_group) {
  g = Gemm2Params{};
  g.W = (const u16*)W; g.bias = bias; g.out = out; g.gn_partial = gn_partial;
  g.B = B; g.Lout = Lout; g.N = N; g.Npad = N; g.K = Kpad; g.Kpad = Kpad; g.ldo = N; g.o_batch_stride = (long long)Lout * N;
  g.alpha = 1.0f; g.epi = EPI_NONE; g.out_f32 = out_f32; g.gn_group = gn_group; g.nsplit = 0;
  g.w_records = (int)((long long)N * Kpad * 2);
  g.gn_slots = 2 * ((Lout + 127) / 128);
  const int osz = out_f32 == 1 ? 4 : 2;
  g.vec_ok = ((((uintptr_t)out) % 16) == 0 && ((N * osz) % 16) == 0) ? 1 : 0;
  g.p_drop = 0.f; g.seed = 0u; g.aux = nullptr; g.out2 = nullptr; g.resid = nullptr;
}

// Conv1d(Cin -> N, ksize, stride, zero padding `pad`) on x = GELU(sc1 * x1 + sh1 [+ sc2 * x2 + sh2]) (see conv16p above).
//   x1, x2 [B, Lin, Cin] 16-bit channels-last raw conv outputs; sc / sh [B, Cin] fp32 (sfm_gn_finalize)
//   W [N][ksize * Cin] 16-bit tap-major (the layout sfm_gemm16 takes), bias [N] fp32; out [B, Lout, N] (out_f32 as sfm_gemm16);
//   gn_partial [B][2 ceil(Lout / 128)][N / gn_group][2] or NULL
//   Ws / bias_s / out_s / gn_partial_s: optional fused Conv1d(Cin -> N, 1, stride 2) on the same x (N = 128, ksize 7 only)
// Supported (the PerceptionAgent's layers): Cin % 64 == 0 and (ksize, stride, pad, N, inputs) in {(7, 2, 3, 128 + fused skip, 1 | 2),
// (7, 2, 3, 256, 2), (3, 1, 1, 128 | 256, 1), (5, 2, 2, 256, 2), (1, 2, 0, 256, 2)}; anything else returns SFM_ERR_SHAPE.
static int conv16p_go(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2, const float* sh2,
                      const void* W, const float* bias, void* out, float* gn_partial, const void* Ws, const float* bias_s,
                      void* out_s, float* gn_partial_s, int B, int Lin, int Cin, int N, int ksize, int stride, int pad,
                      int out_f32, int gn_group, int dtype, void* stream, const int* lin_tab, const int* lout_tab) {
  if (!x1 || !sc1 || !sh1 || !W || !out) return SFM_ERR_ARG;
  if ((x2 != nullptr) != (sc2 != nullptr) || (x2 != nullptr) != (sh2 != nullptr)) return SFM_ERR_ARG;
  if (B <= 0 || Lin <= 0 || Cin <= 0 || (Cin % 64) != 0 || (N != 128 && N != 256)) return SFM_ERR_SHAPE;
  if (out_f32 < 0 || out_f32 > 2) return SFM_ERR_SHAPE;
  if ((gn_partial || gn_partial_s) && gn_group != 8 && gn_group != 16 && gn_group != 32) return SFM_ERR_SHAPE;
  if ((long long)Lin * Cin * 2 >= (1LL << 31) || (long long)N * ksize * Cin * 2 >= (1LL << 31)) return SFM_ERR_SHAPE;
  if ((long long)((Lin + 2 * pad - ksize) / stride + 1) * N * 4 >= (1LL << 31)) return SFM_ERR_SHAPE;       // 32-bit store offsets per utterance
  const int Lout = (Lin + 2 * pad - ksize) / stride + 1;
  if (Lout <= 0) return SFM_ERR_SHAPE;
  const bool skip = Ws != nullptr;
  if (skip && (!out_s || N != 128 || ksize != 7 || stride != 2)) return SFM_ERR_SHAPE;
  if ((((uintptr_t)out) % 16) != 0 || (out_s && (((uintptr_t)out_s) % 16) != 0)) return SFM_ERR_SHAPE;   // 16-byte row stores
  ConvPParams p{};
  convp_fill(p.g, W, bias, out, gn_partial, B, Lout, N, ksize * Cin, out_f32, gn_group);
  if (skip) convp_fill(p.gs, Ws, bias_s, out_s, gn_partial_s, B, Lout, N, Cin, out_f32, gn_group);
  p.x1 = (const u16*)x1; p.sc1 = sc1; p.sh1 = sh1; p.x2 = (const u16*)x2; p.sc2 = sc2; p.sh2 = sh2;
  p.Lin = Lin; p.Cin = Cin; p.pad = pad; p.nMt = (Lout + 127) / 128; p.x_batch_stride = (long long)Lin * Cin;
  hipStream_t st = (hipStream_t)stream;
  const bool two = x2 != nullptr;
  const int key = ksize * 100 + stride * 10 + pad;
  // the layer shapes of the PerceptionAgent (agents/perception.py:160-171 with encoder_channels 256); anything else: SFM_ERR_SHAPE
#define CONVP_GO(TT)                                                                                       \
  if (key == 723 && N == 128 && skip) return two ? launch_convp<TT, 7, 2, 1, true, true>(p, st, lin_tab, lout_tab) : launch_convp<TT, 7, 2, 1, true, false>(p, st, lin_tab, lout_tab); \
  if (key == 723 && N == 256 && !skip && two) return launch_convp<TT, 7, 2, 2, false, true>(p, st, lin_tab, lout_tab);        \
  if (key == 311 && N == 128 && !two) return launch_convp<TT, 3, 1, 1, false, false>(p, st, lin_tab, lout_tab);                \
  if (key == 311 && N == 256 && !two) return launch_convp<TT, 3, 1, 2, false, false>(p, st, lin_tab, lout_tab);                \
  if (key == 522 && N == 256 && two) return launch_convp<TT, 5, 2, 2, false, true>(p, st, lin_tab, lout_tab);                  \
  if (key == 120 && N == 256 && two) return launch_convp<TT, 1, 2, 2, false, true>(p, st, lin_tab, lout_tab);
  if (dtype == SFM_DT_BF16) { CONVP_GO(BF16) }
  if (dtype == SFM_DT_F16) { CONVP_GO(F16) }
#undef CONVP_GO
  return SFM_ERR_SHAPE;
}

extern "C" int sfm_conv16p(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2, const float* sh2,
                           const void* W, const float* bias, void* out, float* gn_partial, const void* Ws, const float* bias_s,
                           void* out_s, float* gn_partial_s, int B, int Lin, int Cin, int N, int ksize, int stride, int pad,
                           int out_f32, int gn_group, int dtype, void* stream) {
  return conv16p_go(x1, sc1, sh1, x2, sc2, sh2, W, bias, out, gn_partial, Ws, bias_s, out_s, gn_partial_s, B, Lin, Cin, N, ksize, stride,
                    pad, out_f32, gn_group, dtype, stream, nullptr, nullptr);
}

// sfm_conv16p on ragged rows.  Every buffer has the dense layout of the LONGEST row: x1, x2 [B, Lin, Cin], out [B, Lout, N] with
// Lout = (Lin + 2 pad - ksize) / stride + 1, gn_partial [B][2 ceil(Lout / 128)][N / gn_group][2] ZERO-FILLED by the caller.
// Utterance b has lin_tab[b] <= Lin input rows and lout_tab[b] = (lin_tab[b] + 2 pad - ksize) / stride + 1 output rows (int32 [B],
// device).  Input rows from lin_tab[b] on are never read: they are the conv's zero edge.  Output rows from lout_tab[b] on are not
// written, nor are the partial slots of the tiles past them.  What is written for utterance b is what sfm_conv16p writes for
// that utterance alone (B = 1, Lin = lin_tab[b]), bit for bit.  Same shapes as sfm_conv16p; the skip and two-input forms included.
extern "C" int sfm_conv16p_varlen(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2,
                                  const float* sh2, const void* W, const float* bias, void* out, float* gn_partial, const void* Ws,
                                  const float* bias_s, void* out_s, float* gn_partial_s, const int* lin_tab, const int* lout_tab,
                                  int B, int Lin, int Cin, int N, int ksize, int stride, int pad, int out_f32, int gn_group,
                                  int dtype, void* stream) {
  if (!lin_tab || !lout_tab) return SFM_ERR_ARG;
  return conv16p_go(x1, sc1, sh1, x2, sc2, sh2, W, bias, out, gn_partial, Ws, bias_s, out_s, gn_partial_s, B, Lin, Cin, N, ksize, stride,
                    pad, out_f32, gn_group, dtype, stream, lin_tab, lout_tab);
}
