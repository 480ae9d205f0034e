// The text of the four-chain MFMA BiLSTM kernel, included by lstm.hip once per form (no include guard):
//   LSTM_VARLEN 0: bilstm_layer16_mfma_kernel - every chain has T steps;
//   LSTM_VARLEN 1: bilstm_layer16_mfma_varlen_kernel - ragged rows.  T = rows per chain of xg and out; chain b runs
//     Tj = ttab[b] <= T steps - forward 0 .. Tj - 1, reverse from Tj - 1 down - while the workgroup steps until the longest of
//     its four chains is done (Tw).  A finished chain's lanes go on through the barriers and the MFMAs, whose result columns
//     are independent, re-reading their last xg row, and store nothing; afterwards every lane writes zeros into its column of
//     the rows from Tj on.  Rows of xg from Tj on are never read.
// LSTM_TJ / LSTM_TW / LSTM_STORES(s): the lane's chain length, the workgroup's step count, whether step s stores - T, T and
// `live` in the dense form, whose text is otherwise the text as it always was.
template <int OUT>
#if LSTM_VARLEN
#define LSTM_TJ Tj
#define LSTM_TW Tw
#define LSTM_STORES(s) (live && (s) < Tj)
__global__ __launch_bounds__(512) void bilstm_layer16_mfma_varlen_kernel(const float* __restrict__ xg, const float* __restrict__ whh,
                                                                         void* __restrict__ out, long long ldo, int B, int T,
                                                                         const int* __restrict__ ttab) {
#else
#define LSTM_TJ T
#define LSTM_TW T
#define LSTM_STORES(s) live
__global__ __launch_bounds__(512) void bilstm_layer16_mfma_kernel(const float* __restrict__ xg, const float* __restrict__ whh,
                                                                  void* __restrict__ out, long long ldo, int B, int T) {
#endif
  typedef typename std::conditional<OUT == LSTM_OUT_F32, float, u16>::type out_t;
  constexpr int H = 128;
  constexpr int CS = 2 * H + 64;                             // byte stride of a chain's h
  constexpr int BUF = LSTM_MFMA_CHAINS * CS;                 // bytes of one buffer
  __shared__ __attribute__((aligned(16))) uint32_t hs[2 * BUF / 4];
  const int tid = threadIdx.x;
  const int u = tid >> 2, j = tid & 3;                       // hidden unit (16 per wave); gate row of A = chain column of B and D
  const int dir = blockIdx.x;
  const int chain = blockIdx.y * LSTM_MFMA_CHAINS + j;
  const bool live = chain < B;
  const int b = live ? chain : B - 1;
#if LSTM_VARLEN
  const int Tj = min(max(ttab[b], 1), T);
  int Tw = 1;
  for (int k = 0; k < LSTM_MFMA_CHAINS; ++k) {
    const int ck = blockIdx.y * LSTM_MFMA_CHAINS + k;
    if (ck < B) Tw = max(Tw, min(ttab[ck], T));
  }
#endif
  lstm_h4 w[H / 4];
  {
    const float* wr = whh + ((long long)dir * 4 * H + j * H + u) * H;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(wr + 32 * q + 4 * i);
        w[8 * q + i] = lstm_h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      }
      __builtin_amdgcn_sched_barrier(0);                     // a quarter of the fp32 row in flight at a time
    }
  }
  for (int i = tid; i < 2 * BUF / 4; i += 512) hs[i] = 0u;
  __syncthreads();
  float c = 0.f;
  const int t0 = dir ? (LSTM_TJ - 1) : 0, dt = dir ? -1 : 1;
  const float* xb = xg + (((long long)b * T + t0) * 2 + dir) * (4 * H) + u;      // step s: + s * dt * 8H, gate g: + g * H
  out_t* ob = reinterpret_cast<out_t*>(out) + ((long long)b * T + t0) * ldo + dir * H + u;
  const long long xstep = (long long)dt * (8 * H), ostep = (long long)dt * ldo;
  const uint32_t hbase = (uint32_t)(uintptr_t)(lds_ptr_t)&hs[0];
  const int grp = (tid >> 4) & 3;                            // 16-lane group of the wave
  const uint32_t hread = hbase + j * CS + grp * 16;           // this column's chain, this group's 8 halves of every 32
  const uint32_t hslot = hbase + j * CS + u * 2;              // where this lane publishes its h
  // xg runs PF steps ahead of its use (a step is shorter than an HBM miss): ring slot s % PF.  Every step issues its four loads -
  // past the end it re-reads step T - 1 - so that the wait in front of a use can be a counted one: the main loop below has
  // no branch that would change how many loads follow the one waited for.
  constexpr int PF = 4;
  f32x4 xr[PF];
  auto fetch = [&](f32x4& x, int s) {
    const float* xs = xb + (s < LSTM_TJ ? s : LSTM_TJ - 1) * xstep;
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = xs[g * H];
  };
#pragma unroll
  for (int i = 0; i < PF; ++i) fetch(xr[i], i);
  // one time step; `par` = s & 1 is the buffer read, the other one is written
  auto step = [&](f32x4& x, int s, int par) {
    f32x4 a0 = x, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
    fetch(x, s + PF);
    const uint32_t hc = hread + (uint32_t)(par * BUF);
    u32x4 hv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(hv[q]) : "v"(hc), "n"(q * 64) : "memory");
    // read q (k = 32q .. 32q + 31 over the four groups) passes through its counted wait, then feeds two MFMAs of each
    // accumulator in k order: BLGP 4 + g hands group g's B operand to all four groups.  The scheduling barrier keeps the next
    // wait from rising above these MFMAs.
#define LSTM_MFMA_PAIR(q, g, acc0, acc1)                                                                                         \
    acc0 = __builtin_amdgcn_mfma_f32_4x4x4f16(w[8 * q + 2 * g], __builtin_shufflevector(p, p, 0, 1, 2, 3), acc0, 0, 0, 4 + g);   \
    acc1 = __builtin_amdgcn_mfma_f32_4x4x4f16(w[8 * q + 2 * g + 1], __builtin_shufflevector(p, p, 4, 5, 6, 7), acc1, 0, 0, 4 + g);
#define LSTM_MFMA_GROUP(q, left)                                                                                                 \
    {                                                                                                                            \
      asm volatile("s_waitcnt lgkmcnt(" #left ")" : "+v"(hv[q])::"memory");                                                      \
      const f16x8_t p = __builtin_bit_cast(f16x8_t, hv[q]);                                                                      \
      LSTM_MFMA_PAIR(q, 0, a0, a1)                                                                                               \
      LSTM_MFMA_PAIR(q, 1, a2, a3)                                                                                               \
      LSTM_MFMA_PAIR(q, 2, a0, a1)                                                                                               \
      LSTM_MFMA_PAIR(q, 3, a2, a3)                                                                                               \
    }                                                                                                                            \
    __builtin_amdgcn_sched_barrier(0);
    LSTM_MFMA_GROUP(0, 3)
    LSTM_MFMA_GROUP(1, 2)
    LSTM_MFMA_GROUP(2, 1)
    LSTM_MFMA_GROUP(3, 0)
#undef LSTM_MFMA_GROUP
#undef LSTM_MFMA_PAIR
    const f32x4 pre = (a0 + a1) + (a2 + a3);
    const float ig = fast_sigmoid(pre[0]), fg = fast_sigmoid(pre[1]);
    const float cg = 2.0f * fast_sigmoid(2.0f * pre[2]) - 1.0f, og = fast_sigmoid(pre[3]);
    c = fg * c + ig * cg;
    float h = og * (2.0f * fast_sigmoid(2.0f * c) - 1.0f);
    asm volatile("" : "+v"(h));                                // the fp32 h is formed first: LDS gets (_Float16) of the value stored
    const uint32_t hb = (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)h);
    asm volatile("ds_write_b16 %0, %1" ::"v"(hslot + (uint32_t)((par ^ 1) * BUF)), "v"(hb) : "memory");
    if (LSTM_STORES(s)) {
      if constexpr (OUT == LSTM_OUT_F32) ob[s * ostep] = h;
      else if constexpr (OUT == SFM_DT_F16) ob[s * ostep] = (u16)hb;
      else ob[s * ostep] = BF16::from_f32(h);
    }
    // LDS-only barrier: the xg loads in flight and the store of h are not waited for
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  int s0 = 0;
  for (; s0 + PF <= LSTM_TW; s0 += PF) {                             // PF is even: the parity of step s0 + i is that of i
    step(xr[0], s0, 0);
    step(xr[1], s0 + 1, 1);
    step(xr[2], s0 + 2, 0);
    step(xr[3], s0 + 3, 1);
  }
  if (s0 < LSTM_TW) step(xr[0], s0, 0);                        // the T % PF steps left
  if (s0 + 1 < LSTM_TW) step(xr[1], s0 + 1, 1);
  if (s0 + 2 < LSTM_TW) step(xr[2], s0 + 2, 0);
#if LSTM_VARLEN
  if (live) {                                                  // rows Tj .. T - 1 of this lane's column: zeros
    out_t* oz = reinterpret_cast<out_t*>(out) + (long long)b * T * ldo + dir * H + u;
    for (int t = Tj; t < T; ++t) oz[t * ldo] = (out_t)0;
  }
#endif
}
#undef LSTM_TJ
#undef LSTM_TW
#undef LSTM_STORES
