// PerceptionAgent latent heads + the time pooling that follows them in the fused path, one launch:
//     raw[b, t, :] = xd[b, t, :256] W^T + bias            (agents/perception.py:183-199: real_proj | imag_proj 1x1 convs, stacked)
//     partial sums of raw, raw^2 per (utterance, row tile, group)  -> GroupNorm statistics of the heads (gn_finalize as before)
//     pooled[b, i, :] = mean over t in [floor(i Tin / Tout), ceil((i + 1) Tin / Tout)) of raw[b, t, :]      (glue G1)
// The GroupNorm that follows the heads has no activation, so it is affine per (utterance, channel) and commutes with the
// average: the caller applies it to `pooled` (sfm_pool_time_affine16 with Tin == Tout).  The full-rate raw tensor
// ([B, Tpa, 512] 16-bit: 670 MB written and 670 MB read back by the pooling pass at B 256 x 512 frames) never exists.
// Kernel = csrc/lin256.hip's scheme (A tile resident in registers, W through a 3-stage LDS-DMA ring, epilogue of a 64-column chunk
// under the next chunk's MFMAs) with row tiles cut at POOLED-FRAME boundaries of one utterance: a workgroup owns `fpt` pooled
// frames = at most 128 input rows.  A chunk's results cross a double-buffered 16-bit LDS image as in lin256 (the rounding the
// un-fused pair applies when it writes the raw tensor); instead of row stores, 16 lanes per pooled frame average the window's
// rows out of the image in fp32.  A row shared by two neighbouring windows at a
// tile boundary is computed by both tiles and counted in the statistics of the first only.  Statistics: fixed summation order
// (wave reduction, then the four row groups of the workgroup in order): bit-reproducible.
#include "sfm_common.h"

#define HP_BM 128
#define HP_K 256
#define HP_STAGE 32768
#define HP_NSTAGE 3
#define HP_IMG 16384

#define HP_VARLEN 0
#include "headpool_kernel.h"                                       // headpool_kernel: the dense form
#undef HP_VARLEN
#define HP_VARLEN 1
#include "headpool_kernel.h"                                       // headpool_varlen_kernel: (Tin, Tout, tiles) per utterance
#undef HP_VARLEN


// frames per tile for a (Tin, Tout) pair: the largest f <= 32 whose window union never exceeds 128 rows; 0 = not supported
extern "C" int sfm_headpool_frames_per_tile(int Tin, int Tout) {
  if (Tin <= 0 || Tout <= 0 || Tin < Tout) return 0;
  for (int f = 32; f >= 1; --f) {
    bool ok = true;
    for (int i0 = 0; i0 < Tout && ok; i0 += f) {
      const int i1 = i0 + f < Tout ? i0 + f : Tout;
      const long long lo = ((long long)i0 * Tin) / Tout, hi = (((long long)i1) * Tin + Tout - 1) / Tout;
      if (hi - lo > HP_BM) ok = false;
    }
    if (ok) return f;
  }
  return 0;
}

// xd [B, Tin, lda] 16-bit (256 valid columns), W [NW, 256] 16-bit, bias [NW] fp32 or NULL ->
//   pooled [B, Tout, ldp] 16-bit (NW columns): the time-pooled RAW head outputs,
//   gn_partial [B, P, NW / gcols, 2] fp32 with P = ceil(Tout / sfm_headpool_frames_per_tile(Tin, Tout)): sum and sum of squares of the
//   full-rate raw outputs per (utterance, tile, group of gcols channels) - the operand sfm_gn_finalize reduces.
extern "C" int sfm_headpool(const void* xd, const void* W, const float* bias, void* pooled, float* gn_partial, int B, int Tin,
                            int Tout, int NW, int lda, int ldp, int gcols, int dtype, void* stream) {
  if (!xd || !W || !pooled || !gn_partial) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  const int fpt = sfm_headpool_frames_per_tile(Tin, Tout);
  if (B <= 0 || fpt <= 0 || NW <= 0 || (NW % 64) != 0 || NW > 1024 || gcols != 16 || lda < HP_K || (lda % 8) != 0 || (ldp % 4) != 0 ||
      ldp < NW)
    return SFM_ERR_SHAPE;
  const int P = (Tout + fpt - 1) / fpt;
  const long long p_bytes = (long long)B * Tout * ldp * 2, a_b = (long long)Tin * lda * 2;
  if (p_bytes >= (1LL << 31) || a_b >= (1LL << 31) || (long long)B * P > 2147483647LL) return SFM_ERR_SHAPE;
  const int ngr = NW / gcols;
  const int lds = HP_NSTAGE * HP_STAGE + 2 * HP_IMG + NW * 4 + 4 * ngr * 2 * 4;
  const int w_bytes = NW * HP_K * 2;
  dim3 grid(B * P), block(512);
  hipStream_t st = (hipStream_t)stream;
#define HP_GO(TT) SFM_LAUNCH_LDS((headpool_kernel<TT>), grid, block, lds, st, (const u16*)xd, (const u16*)W, bias, (u16*)pooled, gn_partial, \
                                 Tin, Tout, NW, lda, ldp, fpt, P, gcols, w_bytes, (int)p_bytes)
  if (dtype == SFM_DT_F16) HP_GO(F16);
  else HP_GO(BF16);
#undef HP_GO
  return SFM_OK;
}

// sfm_headpool on ragged rows: xd [B, TinS, lda], pooled [B, ToutS, ldp], gn_partial [B, PS, NW / gcols, 2] ZERO-FILLED by the
// caller, tab int32 [B][4] (device) = (Tin_b, Tout_b, sfm_headpool_frames_per_tile(Tin_b, Tout_b), ceil(Tout_b / that)) with
// Tin_b <= TinS, Tout_b <= ToutS and at most PS tiles.  Rows of xd from Tin_b on are never read; pooled rows from Tout_b on are
// written as zeros; the partial slots of the tiles from P_b on are not written.  What utterance b gets is what sfm_headpool
// writes for it alone (B = 1, Tin_b, Tout_b), bit for bit.
extern "C" int sfm_headpool_varlen(const void* xd, const void* W, const float* bias, void* pooled, float* gn_partial, const int* tab,
                                   int B, int TinS, int ToutS, int PS, int NW, int lda, int ldp, int gcols, int dtype, void* stream) {
  if (!xd || !W || !pooled || !gn_partial || !tab) return SFM_ERR_ARG;
  if (dtype != SFM_DT_BF16 && dtype != SFM_DT_F16) return SFM_ERR_ARG;
  if (B <= 0 || TinS <= 0 || ToutS <= 0 || PS <= 0 || NW <= 0 || (NW % 64) != 0 || NW > 1024 || gcols != 16 || lda < HP_K ||
      (lda % 8) != 0 || (ldp % 4) != 0 || ldp < NW || (((uintptr_t)pooled) % 8) != 0)
    return SFM_ERR_SHAPE;
  const long long p_bytes = (long long)B * ToutS * ldp * 2, a_b = (long long)TinS * lda * 2;
  if (p_bytes >= (1LL << 31) || a_b >= (1LL << 31) || (long long)B * PS > 2147483647LL) return SFM_ERR_SHAPE;
  const int ngr = NW / gcols;
  const int lds = HP_NSTAGE * HP_STAGE + 2 * HP_IMG + NW * 4 + 4 * ngr * 2 * 4;
  const int w_bytes = NW * HP_K * 2;
  dim3 grid(B * PS), block(512);
  hipStream_t st = (hipStream_t)stream;
#define HP_GO(TT) SFM_LAUNCH_LDS((headpool_varlen_kernel<TT>), grid, block, lds, st, (const u16*)xd, (const u16*)W, bias, (u16*)pooled, \
                                 gn_partial, tab, NW, lda, ldp, gcols, w_bytes, (int)p_bytes, TinS, ToutS, PS)
  if (dtype == SFM_DT_F16) HP_GO(F16);
  else HP_GO(BF16);
#undef HP_GO
  return SFM_OK;
}
