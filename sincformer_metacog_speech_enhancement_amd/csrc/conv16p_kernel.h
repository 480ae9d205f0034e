// The text of the conv16p kernel, included by conv16p.hip once per form (no include guard):
//   CONVP_VARLEN 0: conv16p_kernel(ConvPParams p) - every utterance has p.Lin input rows and p.g.Lout output rows;
//   CONVP_VARLEN 1: conv16p_varlen_kernel(ConvPParams p, lin_tab, lout_tab) - ragged rows.  p describes the buffers, laid out
//     for the LONGEST row (p.x_batch_stride, g.o_batch_stride, g.gn_slots, p.nMt); utterance b has lin_tab[b] input rows and
//     lout_tab[b] output rows.  The workgroup overwrites p.Lin, p.g.Lout and p.gs.Lout of ITS copy of p with its utterance's
//     values, so the descriptors, the position test, rowok and FULL below take them, and it leaves before it stages anything
//     when its tile starts at or past lout_tab[b].
// The dense form is the text as it always was: the ragged one adds the block under `#if CONVP_VARLEN` and nothing else.
template <class T, int KS, int STRIDE, int NPASS, bool SKIP, bool TWO_IN>
#if CONVP_VARLEN
__global__ __launch_bounds__(256, 2) void conv16p_varlen_kernel(ConvPParams p, const int* __restrict__ lin_tab,
                                                               const int* __restrict__ lout_tab) {
  {
    const int total = gridDim.x, q = total >> 3, r = total & 7, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int idv = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;      // the XCD-aware order below
    const int bv = idv / p.nMt;
    const int lout = min(max(lout_tab[bv], 0), p.g.Lout);
    if ((idv - bv * p.nMt) * 128 >= lout) return;      // workgroup-uniform, ahead of every barrier and every LDS write
    p.Lin = min(max(lin_tab[bv], 0), p.Lin);
    p.g.Lout = lout;
    p.gs.Lout = lout;
  }
#else
__global__ __launch_bounds__(256, 2) void conv16p_kernel(ConvPParams p) {
#endif
  constexpr int R = 127 * STRIDE + KS;                 // input rows of a 128-row output tile
  constexpr int PLANES = (STRIDE == 2 && KS > 1) ? 2 : 1;
  constexpr int PR = (((STRIDE == 2) ? (R + 1) / 2 : R) + 7) / 8 * 8;               // rows per plane (whole 1-KB DMA pieces)
  constexpr int PATCH = PLANES * PR * 128;             // bytes
  constexpr int WT = 128 * 128;                        // one weight tile: 128 output channels x 64 k
  constexpr int TPS = NPASS * KS + (SKIP ? 1 : 0);     // weight tiles per 64-channel slab
  static_assert(!SKIP || NPASS == 1, "the fused skip conv needs N = 128");
  static_assert(PATCH + 2 * WT >= 4 * 9216, "epilogue images fit in the patch + ring area");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* ring = smem + PATCH;                  // 2 weight tiles; TWO_IN: also the landing area of the second raw input
  constexpr int RING = (TWO_IN && PATCH > 2 * WT) ? PATCH : 2 * WT;
  float* bias_s = reinterpret_cast<float*>(smem + PATCH + RING);     // [256 main | 128 skip]: what the accumulators start from

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hl = lane >> 5;

  for (int i = tid; i < NPASS * 128; i += 256) bias_s[i] = p.g.bias ? p.g.bias[i] : 0.f;
  if (SKIP && tid < 128) bias_s[256 + tid] = p.gs.bias ? p.gs.bias[tid] : 0.f;
  int id = blockIdx.x;                                 // XCD-aware order: neighbouring tiles (shared halo rows) on one XCD
  {
    const int total = gridDim.x, q = total >> 3, r = total & 7, xcd = id & 7, slot = id >> 3;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int mtile = id % p.nMt, b = id / p.nMt;
  const int l0 = mtile * 128;
  const int nslab = p.Cin >> 6;
  const int Q = nslab * TPS;                           // weight tiles of this output tile

  auto w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.g.W, 0, p.g.w_records, 0x00020000);
  auto ws_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(SKIP ? p.gs.W : p.g.W), 0, SKIP ? p.gs.w_records : p.g.w_records, 0x00020000);
  // LDS-DMA lane coordinates of a weight tile (8 rows x 128 B per instruction, 4 instructions per wave)
  int b_row[4], b_swz[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b_row[i] = (wave * 4 + i) * 8 + (lane >> 3);
    b_swz[i] = ((lane & 7) ^ ((b_row[i] >> 1) & 7)) * 8;
  }
  // weight tile q of the sequence: slab = q / TPS; within the slab: (pass, tap) main tiles, then the skip tile
  auto issue_w = [&](int q) {
    const int slab = q / TPS, j = q - slab * TPS;
    unsigned char* dst = ring + (q & 1) * WT;
    if (SKIP && j == TPS - 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ws_rs, (lds_ptr_t)(dst + (wave * 4 + i) * 1024), 16,
                                                 (b_row[i] * p.gs.Kpad + slab * 64 + b_swz[i]) * 2, 0, 0, 0);
    } else {
      const int np = j / KS, t = j - np * KS;
      const int koff = t * p.Cin + slab * 64;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_ptr_t)(dst + (wave * 4 + i) * 1024), 16,
                                                 ((np * 128 + b_row[i]) * p.g.Kpad + koff + b_swz[i]) * 2, 0, 0, 0);
    }
  };

  // Started from the bias behind the first patch (convp_acc_init, under `if (slab == 0)` in the slab loop).  Until then their
  // contents do not matter, but a zero fill here is not dead to the compiler (the overwrite is conditional): it cost 64 x NPASS
  // (+ 64 for the skip tile) v_mov per lane and tile.  The empty asm defines each register tuple with NO instruction; left
  // plainly uninitialised the compiler peels the first slab instead and spills in the k 7 + skip kernels.
  f32x16 acc[NPASS][2][2], accs[2][2];
#pragma unroll
  for (int n = 0; n < NPASS; ++n)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("" : "=v"(acc[n][i][j]));
  if (SKIP) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("" : "=v"(accs[i][j]));
  }

  int fb_off[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = wn * 64 + j * 32 + l31;
#pragma unroll
    for (int s = 0; s < 4; ++s) fb_off[j][s] = row * 128 + (((2 * s + hl) ^ ((row >> 1) & 7)) << 4);
  }

  // ---- patch staging.  (1) the RAW rows of the slab go global -> LDS by LDS-DMA, all at once (33 KB in flight per workgroup:
  //      with register staging three dependent global round trips per slab left ~1 TB/s of read stream; rows outside
  //      [0, Lin) and LDS rows beyond the patch are out of the descriptor's range and arrive as zeros); the second input of a
  //      residual block lands in the weight ring, which is idle until the transform is done.  (2) every thread transforms
  //      its 16-byte chunks IN PLACE (scale / shift [+ second input] -> GELU -> 16 bit); zero-filled padding rows stay zero,
  //      as the conv's zero padding of x requires.  The chunk swizzle is applied on the DMA's source address, and
  //      ((row >> 1) & 7) of a thread's rows (row = tid / 8 + 32 i) is constant, so a thread owns the same 8 channels in every
  //      row: their scale / shift sit in registers. ----
  constexpr int JSTEP = (PLANES == 1 && STRIDE == 2) ? 2 : 1;        // k = 1, stride 2: only the even input rows are read
  constexpr int LROWS = PLANES * PR;                                 // LDS rows of the patch
  constexpr int NPIECE = (LROWS + 7) / 8;                            // 1-KB DMA pieces
  auto x1_rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x1 + (long long)b * p.x_batch_stride), 0, p.Lin * p.Cin * 2, 0x00020000);
  auto x2_rs = __builtin_amdgcn_make_buffer_rsrc((void*)((TWO_IN ? p.x2 : p.x1) + (long long)b * p.x_batch_stride), 0,
                                                 p.Lin * p.Cin * 2, 0x00020000);
  // input position of LDS row lr (or -1): plane / index de-interleaving for stride 2
  auto row_pos = [&](int lr) {
    const int plane = (PLANES == 2) ? (lr >= PR ? 1 : 0) : 0;
    const int idx = lr - plane * PR;
    const int j = (PLANES == 2) ? 2 * idx + plane : idx * JSTEP;
    const int pos = l0 * STRIDE - p.pad + j;
    return (lr < LROWS && j < R && pos >= 0 && pos < p.Lin) ? pos : -1;
  };
  // the same as ranges: LDS rows [tr_lo, tr_hi) of plane pl are the ones with row_pos >= 0 (j = JS idx + pl in [jlo, jhi))
  int tr_lo[PLANES], tr_hi[PLANES];
  {
    constexpr int JS = (PLANES == 2) ? 2 : JSTEP;
    const int base = l0 * STRIDE - p.pad;
    const int jlo = max(-base, 0), jhi = min(p.Lin - base, R);
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) {
      tr_lo[pl] = pl * PR + (jlo - pl + JS - 1) / JS;                // jlo - pl + JS - 1 >= 0
      tr_hi[pl] = pl * PR + min((max(jhi - pl, 0) + JS - 1) / JS, PR);
    }
  }
  const int sp_ = tid & 7, srow = tid >> 3;
  const int sc_ = sp_ ^ ((srow >> 1) & 7);                           // logical chunk (8 channels) this thread owns in every row
  auto stage_patch = [&](int slab) {
    for (int pc = wave; pc < NPIECE; pc += 4) {
      const int lr = pc * 8 + (lane >> 3);
      const int pos = row_pos(lr);
      const int c = (lane & 7) ^ ((lr >> 1) & 7);
      const int voff = pos >= 0 ? (pos * p.Cin + slab * 64 + c * 8) * 2 : -1;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(x1_rs, (lds_ptr_t)(smem + pc * 1024), 16, voff, 0, 0, 0);
      if (TWO_IN) __builtin_amdgcn_raw_ptr_buffer_load_lds(x2_rs, (lds_ptr_t)(ring + pc * 1024), 16, voff, 0, 0, 0);
    }
    const int ch0 = slab * 64 + sc_ * 8;
    float a1[8], d1[8], a2[8];
    {
      const f32x4* ps = reinterpret_cast<const f32x4*>(p.sc1 + (long long)b * p.Cin + ch0);
      const f32x4* ph = reinterpret_cast<const f32x4*>(p.sh1 + (long long)b * p.Cin + ch0);
      const f32x4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { a1[e] = s0[e]; a1[4 + e] = s1[e]; d1[e] = h0[e]; d1[4 + e] = h1[e]; }
      if (TWO_IN) {
        const f32x4* qs = reinterpret_cast<const f32x4*>(p.sc2 + (long long)b * p.Cin + ch0);
        const f32x4* qh = reinterpret_cast<const f32x4*>(p.sh2 + (long long)b * p.Cin + ch0);
        const f32x4 t0 = qs[0], t1 = qs[1], g0 = qh[0], g1 = qh[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { a2[e] = t0[e]; a2[4 + e] = t1[e]; d1[e] += g0[e]; d1[4 + e] += g1[e]; }
      }
    }
    wait_vmcnt<0>();                                   // this wave's pieces have landed ...
    __syncthreads();                                   // ... everyone's have
    // The rows with row_pos >= 0 are one run of consecutive LDS rows per plane, [tr_lo, tr_hi) (wave-uniform, worked out once per
    // tile above); a thread's rows are srow + 32 i, so it walks from its first row at or above tr_lo to tr_hi without a test
    // per chunk.  The rows outside stay the zeros the DMA left: the conv's zero padding.
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll 2
    for (int lr = srow + (max(tr_lo[pl] - srow + 31, 0) & ~31); lr < tr_hi[pl]; lr += 32) {
      unsigned char* q1 = smem + lr * 128 + sp_ * 16;
      const u32x4 v1 = *reinterpret_cast<const u32x4*>(q1);
      u32x4 v2 = {0u, 0u, 0u, 0u};
      if (TWO_IN) v2 = *reinterpret_cast<const u32x4*>(ring + lr * 128 + sp_ * 16);
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (T::id == SFM_DT_F16) {
          // z = x1 * a1 [+ x2 * a2] + d straight from the packed fp16 inputs (mixed-precision FMA: fp16 source halves, fp32
          // coefficients and arithmetic) into a packed fp16 pair: 2 (4) instructions per pair instead of 4 (7)
          uint32_t zpk;
          float t0 = d1[2 * e], t1 = d1[2 * e + 1];
          if (TWO_IN) {
            asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(t0) : "v"(v2[e]), "v"(a2[2 * e]), "v"(d1[2 * e]));
            asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(t1) : "v"(v2[e]), "v"(a2[2 * e + 1]), "v"(d1[2 * e + 1]));
          }
          asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
              "v_fma_mixhi_f16 %0, %1, %4, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
              : "=&v"(zpk) : "v"(v1[e]), "v"(a1[2 * e]), "v"(t0), "v"(a1[2 * e + 1]), "v"(t1));
          o[e] = gelu_lg_h2p(zpk);
          continue;
        }
        // bf16: unpack, fp32 affine and GELU, pack
        float z0 = T::to_f32((u16)(v1[e] & 0xffffu)) * a1[2 * e] + d1[2 * e];
        float z1 = T::to_f32((u16)(v1[e] >> 16)) * a1[2 * e + 1] + d1[2 * e + 1];
        if (TWO_IN) {
          z0 += T::to_f32((u16)(v2[e] & 0xffffu)) * a2[2 * e];
          z1 += T::to_f32((u16)(v2[e] >> 16)) * a2[2 * e + 1];
        }
        o[e] = pack2<T>(gelu_as(z0), gelu_as(z1));
      }
      *reinterpret_cast<u32x4*>(q1) = o;
    }
  };

  // ---- one weight tile against the patch rows of tap `t` ----
  auto mma_tile = [&](int q, int t, f32x16 (&a)[2][2]) {
    const unsigned char* wb = ring + (q & 1) * WT;
    int arow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rw = wm * 64 + i * 32 + l31;
      arow[i] = (PLANES == 2) ? (t & 1) * PR + rw + (t >> 1) : ((STRIDE == 2) ? rw : rw + t);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        fa[i] = *reinterpret_cast<const u32x4*>(smem + arow[i] * 128 + (((2 * s + hl) ^ ((arow[i] >> 1) & 7)) << 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const u32x4*>(wb + fb_off[j][s]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) a[i][j] = T::mfma(fb[j], fa[i], a[i][j]);      // transposed tile: rows of C^T = channels
    }
  };

  if (!TWO_IN) issue_w(0);
  for (int slab = 0; slab < nslab; ++slab) {
    if (slab > 0) __syncthreads();                     // every wave is done reading the previous slab's patch (and weight tiles)
    stage_patch(slab);
    __syncthreads();                                   // patch complete
    const int q0 = slab * TPS;
    if (TWO_IN) issue_w(q0);                           // the ring held the second raw input until now
    if (slab == 0) {                                   // wave-uniform; bias_s was written before the patch's barriers
#pragma unroll
      for (int n = 0; n < NPASS; ++n) convp_acc_init(bias_s + n * 128 + wn * 64, acc[n], hl);
      if (SKIP) convp_acc_init(bias_s + 256 + wn * 64, accs, hl);
    }
#pragma unroll
    for (int j = 0; j < TPS; ++j) {
      const int q = q0 + j;
      wait_ring<0>();                                  // this wave's share of weight tile q has landed, its reads of tile q-1 have returned
      __builtin_amdgcn_s_barrier();                    // ... everyone's have: tile q is complete and tile q-1's slot may be refilled
      // Inside a slab the next tile's refill is UNCONDITIONAL (q + 1 < Q always holds there): behind a conditional refill the
      // compiler no longer knows which LDS-DMA operations are pending at the join and guards the tile's first fragment reads
      // with vmcnt waits of its own - i.e. waits for the refill it has just issued (seen in the ISA of round 3's race hunt).
      // The slab's last tile issues the next slab's first tile AFTER its own reads instead: the patch staging that follows is
      // far longer than a weight tile's latency.
      if (j + 1 < TPS) issue_w(q + 1);
      if (SKIP && j == TPS - 1) {
        mma_tile(q, p.pad, accs);                      // 1x1 stride-2 conv = the centre tap of the same patch
      } else {
        const int np = j / KS, t = j - np * KS;
        if (np == 0) mma_tile(q, t, acc[0]);
        else mma_tile(q, t, acc[NPASS - 1]);
      }
      if (j + 1 == TPS && !TWO_IN && q + 1 < Q) issue_w(q + 1);
    }
  }
  __syncthreads();                                     // the ring becomes the epilogue strips
  unsigned char* img = smem + wave * 9216;             // 64 x 144 B per wave, in the (now free) patch + ring area
#pragma unroll
  for (int n = 0; n < NPASS; ++n) convp_epilogue<T>(p.g, acc[n], img, lane, b, n * 128 + wn * 64, l0 + wm * 64);
  if (SKIP) convp_epilogue<T>(p.gs, accs, img, lane, b, wn * 64, l0 + wm * 64);
}
