// The text of the resident-tap kernel, included by sinc_fir16.hip once per form (no include guard):
//   FIRR_VARLEN 0: sinc_fir16_resident_kernel - every row of sig [B, L] has L samples;
//   FIRR_VARLEN 1: sinc_fir16_resident_varlen_kernel - ragged rows.  Row b of sig [B, Lrow] holds L = lengths[b] valid samples;
//     sig and out keep the row stride Lrow (FIRR_LROW below).  Samples from L on are never read (they stage as the FIR's zero
//     edge), rows of out from L on are not stored, and a workgroup whose first span lies past L leaves before it touches memory:
//     its gn_partial slots keep the caller's zero fill.  Tiles are anchored at the row start, so out and gn_partial of row b
//     are the bits the dense kernel gives for that row alone.
// The dense form is the text as it always was.
template <class T>
#if FIRR_VARLEN
#define FIRR_LROW Lrow
__global__ __launch_bounds__(FIRR_WAVES * 64, 2) void sinc_fir16_resident_varlen_kernel(
    const float* __restrict__ sig, const u16* __restrict__ wsh, void* __restrict__ out, float* __restrict__ gn_partial,
    const int* __restrict__ lengths, int Lrow, int pad, int out_f32, int tiles_per_batch, int spans_per_wg) {
  const int L = min(max(lengths[blockIdx.z], 0), Lrow);
  if ((int)blockIdx.y * spans_per_wg * FIRR_OUT >= L) return;      // workgroup-uniform, ahead of every barrier
#else
#define FIRR_LROW L
__global__ __launch_bounds__(FIRR_WAVES * 64, 2) void sinc_fir16_resident_kernel(const float* __restrict__ sig,
                                                                                const u16* __restrict__ wsh, void* __restrict__ out,
                                                                                float* __restrict__ gn_partial, int L, int pad,
                                                                                int out_f32, int tiles_per_batch, int spans_per_wg) {
#endif
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  u16* Xh = reinterpret_cast<u16*>(dsm);                       // [2][FIRR_SPAN]
  float* img = reinterpret_cast<float*>(Xh + 2 * FIRR_SPAN);   // FIRR_WAVES x [32][68] floats

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hl = lane >> 5;
  const int o = blockIdx.x, b = blockIdx.z;
  const int s0 = blockIdx.y * spans_per_wg;
  const int s1 = min(s0 + spans_per_wg, (L + FIRR_OUT - 1) / FIRR_OUT);
  const float* xb = sig + (long long)b * FIRR_LROW;

  // this shift's taps (hi), as the B fragments of every k-step: registers for the whole life of the wave
  u32x4 wt[2][FIR_KP / 16];
  {
    const u16* src = wsh + (long long)o * 2 * FIR_C * FIR_KP;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < FIR_KP / 16; ++s)
        wt[j][s] = *reinterpret_cast<const u32x4*>(src + (j * 32 + l31) * FIR_KP + s * 16 + 8 * hl);
  }

  constexpr int NT = FIRR_WAVES * 64;
  float xr[FIRR_XPT];
  auto load_span = [&](int m0) {
#pragma unroll
    for (int q = 0; q < FIRR_XPT; ++q) {
      const int i = tid + q * NT;
      const int sidx = m0 + i - pad;
      xr[q] = (i < FIRR_SPAN && sidx >= 0 && sidx < L) ? xb[sidx] : 0.f;
    }
  };
  auto write_span = [&](u16* X) {
#pragma unroll
    for (int q = 0; q < FIRR_XPT; ++q) {
      const int i = tid + q * NT;
      if (i < FIRR_SPAN) X[i] = T::from_f32(xr[q]);
    }
  };
  load_span(s0 * FIRR_OUT);
  write_span(Xh);
  if (s0 + 1 < s1) load_span((s0 + 1) * FIRR_OUT);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int s = 0; s < FIR_KP / 16; ++s) asm volatile("" : "+v"(wt[j][s]));      // loaded here, once: never re-fetched in the loop
  __syncthreads();

  float* im = img + wave * (32 * 68);
  const int xoff = wave * 256 + 8 * l31 + 8 * hl;              // + k0: 16-byte aligned for every lane
  const int c8 = (lane & 7) * 8, rsub = lane >> 3;             // epilogue: 8 channels per lane, 8 rows per pass
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    const u16* X = Xh + cur * FIRR_SPAN;
    const int g = s * FIRR_WAVES + wave;                       // global wave-tile: samples [256 g, 256 g + 256) before the shift
    const int m0 = g * 256;
    if (m0 < L) {                                              // wave-uniform; a tile past L has no row to store and sums to zero
      f32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
      for (int k0 = 0; k0 < FIR_KP; k0 += 16) {
        const u32x4 ah = *reinterpret_cast<const u32x4*>(X + xoff + k0);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[j] = T::mfma(ah, wt[j][k0 / 16], acc[j]);
      }

      // ---- epilogue of sinc_fir16_kernel, unchanged: scale back, per-wave image [32 rows][64 ch], stats, row stores ----
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) im[mfma_row(r, lane) * 68 + j * 32 + l31] = acc[j][r] * (1.0f / 4096.0f);
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      float gsum = 0.f, gsq = 0.f;
#pragma unroll
      for (int r0 = 0; r0 < 32; r0 += 8) {
        const int row = r0 + rsub;
        const int m = m0 + o + 8 * row;                        // output sample of this image row
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(&im[row * 68 + c8]);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(&im[row * 68 + c8 + 4]);
        if (m < L) {
          const float v[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
          for (int e = 0; e < 8; ++e) { gsum += v[e]; gsq += v[e] * v[e]; }
          const long long off = ((long long)b * FIRR_LROW + m) * FIR_C + c8;
          if (out_f32) {
            float* op = reinterpret_cast<float*>(out) + off;
            *reinterpret_cast<f32x4*>(op) = x0;
            *reinterpret_cast<f32x4*>(op + 4) = x1;
          } else {
            u32x4 pk;
#pragma unroll
            for (int e = 0; e < 4; ++e) pk[e] = pack2<T>(v[2 * e], v[2 * e + 1]);
            *reinterpret_cast<u32x4*>(reinterpret_cast<u16*>(out) + off) = pk;
          }
        }
      }
      if (gn_partial) {                                        // GroupNorm(8, 64): one 8-channel chunk = one group
        for (int sh = 8; sh < 64; sh <<= 1) {
          gsum += __shfl_xor(gsum, sh, 64);
          gsq += __shfl_xor(gsq, sh, 64);
        }
        if (lane < 8) {
          const long long tile = (long long)(g >> 3) * 64 + o * 8 + (g & 7);
          const long long slot = (((long long)b * tiles_per_batch + tile) * 8 + lane) * 2;
          gn_partial[slot] = gsum;
          gn_partial[slot + 1] = gsq;
        }
      }
    }
    if (s + 1 < s1) {
      write_span(Xh + (cur ^ 1) * FIRR_SPAN);                  // its last readers passed the barrier that ended span s - 1
      if (s + 2 < s1) load_span((s + 2) * FIRR_OUT);           // lands under the MFMAs of span s + 1
    }
    __syncthreads();                                           // span s + 1 is complete; every reader of span s is done
  }
}
#undef FIRR_LROW
