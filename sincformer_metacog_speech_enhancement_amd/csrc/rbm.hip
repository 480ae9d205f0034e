// RBM pre-training (models/rbm.py of the reference: CD-k, Hinton 2006), exact fp32 on v_mfma_f32_32x32x2_f32 (bit for bit a
// k-ordered fmaf chain: no 16-bit operand anywhere, so the sampling decisions prob > u stay those of the float64 reference).
//
//   rbm_prob_kernel    out[M, N] = sigmoid(A[M, K] op(W) + bias[N]); up: op(W) = W [V, H], down: op(W) = W^T.  Row m of A is
//                      data[rows[m]] (the batch gather happens while A is staged), optionally S = prob > u.
//   rbm_update_kernel  W[i, j] += (lr / B) sum_b (v[b, i] ph[b, j] - nv[b, i] nh[b, j]): ONE accumulation over 2 B terms, k = 2 b
//                      the positive and k = 2 b + 1 the negative one (nh is negated while staged); every element of W belongs to
//                      one workgroup, which reads, adds and writes it once.  The tiles of the first hidden column also own their 32
//                      entries of v_bias and the fp64 partial of sum (v - nv)^2 over their columns, the tiles of the first visible row
//                      their 32 entries of h_bias, both summed in fp64 from the rows staged for the product.  No atomics.
//   rbm_fold_kernel    the partials of an epoch's steps -> the mean over the steps of each step's mean squared error, fixed order.
//
// Grid shape: a step at B = 256 is far from flop-bound (1.56 Gflop), so the tiles are small and K is split over the four waves of
// a workgroup: a 32 x 32 output tile, k-chunks of 256 (update: 128 = 64 batch rows) staged in LDS, wave w multiplies the k pairs
// 8 j + 2 w of every chunk; the four accumulators are added in wave order through LDS.  256 x 594 -> 1024: up 8 x 32 = 256
// workgroups, down 8 x 19 = 152, update 19 x 32 = 608.  A result element is a function of its own row and column only (zero
// padding, fixed k order, fixed wave order): the same bits for a row alone or inside any M, and with `rows` or on a gathered copy.
//
// Row starts are only 4-byte aligned (594 floats): every global access here is one float.
#include "sfm_common.h"

#define RT SFM_RBM_TILE
#define RKC SFM_RBM_KCHUNK     // k staged per pass of the probability kernel
#define RUC (RKC / 2)          // ... of the update: 64 batch rows, positive and negative term interleaved
#define RAS (RKC + 1)          // A tile [row][k]: conflict-free fragment reads down a column of k
#define RBS (RT + 1)           // B tile [k][col]
static_assert(RT == 32 && RKC == 256, "the lane maps below are written for 32 x 32 tiles, 256 threads and these chunk sizes");

struct RbmProbParams {
  const float* data;
  const int* rows;
  const float* W;
  const float* bias;
  float* prob;
  float* sample;
  const double* u;
  long long lda;
  int M, N, K, H, n_rows, mode;
  uint32_t seed;
};

// the four waves' partial tiles -> their sum in wave order, for the element (row, col) of the tile
__device__ __forceinline__ float rbm_wave_fold(const float* red, int row, int col) {
  const int o = row * RBS + col;
  return ((red[o] + red[RT * RBS + o]) + red[2 * RT * RBS + o]) + red[3 * RT * RBS + o];
}

__device__ __forceinline__ void rbm_spill(float* red, const f32x16& acc, int wave, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * RT + mfma_row(r, lane)) * RBS + (lane & 31)] = acc[r];
}

// K is split over the waves in pairs: wave w multiplies k = 8 j + 2 w, 8 j + 2 w + 1 of a chunk, j = 0, 1, ..; a short last chunk
// ends the loop early for all four.  A chunk's loads are all in flight at once (one register each) while the chunk before it is
// multiplied: with one workgroup per CU at B = 256 the loop is bound by that latency, so the chunks are long (3 for K = 594).
template <bool DOWN>
__global__ __launch_bounds__(256) void rbm_prob_kernel(RbmProbParams p) {
  __shared__ float smem[RT * RAS + RKC * RBS];
  __shared__ long long rowoff[RT];
  float* As = smem;
  float* Bs = smem + RT * RAS;
  float* red = smem;                                      // after the loop: 4 x 32 x 33 floats over the A tile
  static_assert(4 * RT * RBS <= RT * RAS, "the fold buffer fits the A tile");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntn = (p.N + RT - 1) / RT;                    // the column tile runs fastest: workgroups are dealt round-robin over the
  const int m0 = (int)(blockIdx.x / ntn) * RT, n0 = (int)(blockIdx.x % ntn) * RT;   // XCDs, and an XCD then keeps to its columns of W
  if (tid < RT) {
    const int m = m0 + tid;
    long long off = -1;                                   // a row beyond M, or an index outside the data, is staged as zeros
    if (m < p.M) {
      const int r = p.rows ? p.rows[m] : m;
      if (r >= 0 && r < p.n_rows) off = (long long)r * p.lda;
    }
    rowoff[tid] = off;
  }
  __syncthreads();

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr int NL = RT * RKC / 256;                      // 32 loads per thread and operand
  float ra[NL], rb[NL];
  const int nkc = (p.K + RKC - 1) / RKC;

  auto load_chunk = [&](int kc) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 256 * i;
      {
        const int row = idx / RKC, k = kc * RKC + (idx % RKC);
        const long long off = rowoff[row];
        ra[i] = (off >= 0 && k < p.K) ? p.data[off + k] : 0.f;
      }
      if (DOWN) {                                         // B[k][n] = W[n][k]: contiguous along k
        const int n = n0 + idx / RKC, k = kc * RKC + (idx % RKC);
        rb[i] = (n < p.N && k < p.K) ? p.W[(long long)n * p.H + k] : 0.f;
      } else {                                            // B[k][n] = W[k][n]: contiguous along n
        const int k = kc * RKC + (idx >> 5), n = n0 + (idx & 31);
        rb[i] = (n < p.N && k < p.K) ? p.W[(long long)k * p.H + n] : 0.f;
      }
    }
  };

  load_chunk(0);
  for (int kc = 0; kc < nkc; ++kc) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 256 * i;
      As[(idx / RKC) * RAS + (idx % RKC)] = ra[i];
      if (DOWN) Bs[(idx % RKC) * RBS + idx / RKC] = rb[i];
      else Bs[(idx >> 5) * RBS + (idx & 31)] = rb[i];
    }
    __syncthreads();
    if (kc + 1 < nkc) load_chunk(kc + 1);
    const int left = p.K - kc * RKC;
    const int nj = ((((left < RKC ? left : RKC) + 7) >> 3) + 3) & ~3;      // in fours (the k beyond K are staged as zeros): four
    for (int j = 0; j < nj; j += 4) {                                        // pairs of LDS reads in flight per wait
      float a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 8 * (j + q) + 2 * wave + (lane >> 5);
        a[q] = As[(lane & 31) * RAS + k];
        b[q] = Bs[k * RBS + (lane & 31)];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
    }
    __syncthreads();
  }

  rbm_spill(red, acc, wave, lane);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i, row = e >> 5, col = e & 31;
    const int m = m0 + row, n = n0 + col;
    if (m < p.M && n < p.N) {
      const float x = rbm_wave_fold(red, row, col) + p.bias[n];
      const float pr = 1.0f / (1.0f + expf(-x));          // exp(-x) = inf gives 0, exp(-x) = 0 gives 1: no NaN at either end
      const unsigned long long idx = (unsigned long long)m * (unsigned)p.N + (unsigned)n;
      p.prob[idx] = pr;
      if (p.mode == SFM_RBM_SAMPLE_REPLAY) p.sample[idx] = ((double)pr > p.u[idx]) ? 1.0f : 0.0f;
      else if (p.mode == SFM_RBM_SAMPLE_COUNTER)
        p.sample[idx] = (sfm_keep_word24(sfm_hash(p.seed, idx >> 3), (uint32_t)(idx & 7ull)) < sfm_keep_threshold(pr)) ? 1.0f : 0.0f;
    }
  }
}

struct RbmUpdateParams {
  const float* data;
  const int* rows;
  const float* ph;
  const float* nv;
  const float* nh;
  float* W;
  float* v_bias;
  float* h_bias;
  double* err_partial;
  long long ldv;
  int B, V, H, n_rows;
  float lr;
};

// the eight parts' column sums [8][32] -> the totals in part order, left in s[0 .. 31]
__device__ __forceinline__ void rbm_fold_parts(double* s, int tid) {
  __syncthreads();
  double t = 0.0;
  if (tid < 32) {
#pragma unroll
    for (int k = 0; k < 8; ++k) t += s[k * 32 + tid];
  }
  __syncthreads();
  if (tid < 32) s[tid] = t;
  __syncthreads();
}

__global__ __launch_bounds__(256) void rbm_update_kernel(RbmUpdateParams p) {
  __shared__ float smem[2 * RUC * RBS];
  __shared__ double sv[8 * 32], sq[8 * 32], sh[8 * 32];
  float* As = smem;                    // [k][i]: v and nv are contiguous along i; k = 2 b: v[b], k = 2 b + 1: nv[b]
  float* Bs = smem + RUC * RBS;        // [k][j]: ph[b], then -nh[b]
  float* red = smem;                   // after the loop
  static_assert(4 * RT * RBS <= 2 * RUC * RBS, "the fold buffer fits the two tiles");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntj = (p.H + RT - 1) / RT;
  const int it = blockIdx.x / ntj, jt = blockIdx.x % ntj;
  const int i0 = it * RT, j0 = jt * RT;
  const bool v_edge = jt == 0, h_edge = it == 0;      // the tiles that own v_bias + error / h_bias entries

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  constexpr int NL = RT * RUC / 256;   // 16 loads per thread and operand
  float ra[NL], rb[NL];
  const int K = 2 * p.B, nkc = (K + RUC - 1) / RUC;
  double dv = 0.0, dq = 0.0, dh = 0.0;

  auto load_chunk = [&](int kc) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 256 * i;
      const int c = idx & 31, k = kc * RUC + (idx >> 5);
      const int b = k >> 1;
      float a = 0.f, w = 0.f;
      if (b < p.B) {
        if (k & 1) {
          if (i0 + c < p.V) a = p.nv[(long long)b * p.V + i0 + c];
          if (j0 + c < p.H) w = -p.nh[(long long)b * p.H + j0 + c];
        } else {
          const int r = p.rows ? p.rows[b] : b;
          if (i0 + c < p.V && r >= 0 && r < p.n_rows) a = p.data[(long long)r * p.ldv + i0 + c];
          if (j0 + c < p.H) w = p.ph[(long long)b * p.H + j0 + c];
        }
      }
      ra[i] = a;
      rb[i] = w;
    }
  };

  load_chunk(0);
  for (int kc = 0; kc < nkc; ++kc) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 256 * i;
      As[(idx >> 5) * RBS + (idx & 31)] = ra[i];
      Bs[(idx >> 5) * RBS + (idx & 31)] = rb[i];
    }
    __syncthreads();
    if (kc + 1 < nkc) load_chunk(kc + 1);
    const int left = K - kc * RUC;
    const int nj = ((((left < RUC ? left : RUC) + 7) >> 3) + 3) & ~3;
    for (int j = 0; j < nj; j += 4) {
      float a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 8 * (j + q) + 2 * wave + (lane >> 5);
        a[q] = As[k * RBS + (lane & 31)];
        b[q] = Bs[k * RBS + (lane & 31)];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
    }
    // the edge tiles sum their columns of (v - nv) / (ph - nh) over the batch from the staged rows, in fp64: thread t takes the
    // rows b = t >> 5 (mod 8) of column t & 31 in ascending order (rows beyond B and columns beyond the width are staged as zeros)
    if (v_edge || h_edge) {
      const int c = tid & 31, part = tid >> 5;
#pragma unroll
      for (int r = 0; r < RUC / 16; ++r) {
        const int k = 2 * (part + 8 * r);
        if (v_edge) {
          const double d = (double)As[k * RBS + c] - (double)As[(k + 1) * RBS + c];
          dv += d;
          dq += d * d;
        }
        if (h_edge) dh += (double)Bs[k * RBS + c] + (double)Bs[(k + 1) * RBS + c];
      }
    }
    __syncthreads();
  }

  rbm_spill(red, acc, wave, lane);
  sv[tid] = dv;
  sq[tid] = dq;
  sh[tid] = dh;
  __syncthreads();
  const float scale = p.lr / (float)p.B;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = tid + 256 * i, row = e >> 5, col = e & 31;
    const int vi = i0 + row, hj = j0 + col;
    if (vi < p.V && hj < p.H) {
      float* w = p.W + (long long)vi * p.H + hj;
      *w = __builtin_fmaf(scale, rbm_wave_fold(red, row, col), *w);
    }
  }

  if (v_edge) {                        // this tile's 32 visible units: v_bias and the reconstruction error
    rbm_fold_parts(sv, tid);
    rbm_fold_parts(sq, tid);
    if (tid < 32 && i0 + tid < p.V) p.v_bias[i0 + tid] = (float)((double)p.v_bias[i0 + tid] + (double)p.lr * sv[tid] / (double)p.B);
    if (tid == 0) {
      double e = 0.0;
      for (int c = 0; c < 32; ++c) e += sq[c];
      p.err_partial[it] = e;
    }
  }
  if (h_edge) {                        // this tile's 32 hidden units: h_bias
    rbm_fold_parts(sh, tid);
    if (tid < 32 && j0 + tid < p.H) p.h_bias[j0 + tid] = (float)((double)p.h_bias[j0 + tid] + (double)p.lr * sh[tid] / (double)p.B);
  }
}

// out[0] = mean over the steps s of (sum_t partial[s][t]) / (B_s V), B_s = the rows of batch s of an epoch of num_samples rows
__global__ __launch_bounds__(256) void rbm_fold_kernel(const double* partial, double* out, int n_steps, int n_tiles, int num_samples,
                                                       int batch_size, int V) {
  __shared__ double part[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int st = tid; st < n_steps; st += 256) {
    double e = 0.0;
    for (int t = 0; t < n_tiles; ++t) e += partial[(long long)st * n_tiles + t];
    const long long left = (long long)num_samples - (long long)st * batch_size;
    const long long Bs_ = left < batch_size ? left : batch_size;
    s += e / ((double)Bs_ * (double)V);
  }
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += part[i];
    out[0] = tot / (double)n_steps;
  }
}

static bool rbm_units_ok(int n_visible, int n_hidden) {
  return n_visible >= 1 && n_hidden >= 1 && n_visible <= SFM_RBM_MAX_UNITS && n_hidden <= SFM_RBM_MAX_UNITS;
}

extern "C" int sfm_rbm_prob(const float* data, const int* rows, const float* W, const float* bias, float* prob, float* sample,
                            const double* u, int M, int n_visible, int n_hidden, int n_rows, long long lda, int down,
                            int sample_mode, unsigned int seed, void* stream) {
  if (!data || !W || !bias || !prob) return SFM_ERR_ARG;
  if (down != 0 && down != 1) return SFM_ERR_ARG;
  if (sample_mode != SFM_RBM_SAMPLE_NONE && sample_mode != SFM_RBM_SAMPLE_REPLAY && sample_mode != SFM_RBM_SAMPLE_COUNTER) return SFM_ERR_ARG;
  if ((sample_mode == SFM_RBM_SAMPLE_NONE) != (sample == nullptr)) return SFM_ERR_ARG;
  if ((sample_mode == SFM_RBM_SAMPLE_REPLAY) != (u != nullptr)) return SFM_ERR_ARG;
  if (M < 1 || n_rows < 1 || !rbm_units_ok(n_visible, n_hidden)) return SFM_ERR_SHAPE;
  const int K = down ? n_hidden : n_visible, N = down ? n_visible : n_hidden;
  if (lda < K || (!rows && M > n_rows)) return SFM_ERR_SHAPE;
  RbmProbParams p;
  p.data = data; p.rows = rows; p.W = W; p.bias = bias; p.prob = prob; p.sample = sample; p.u = u;
  p.lda = lda; p.M = M; p.N = N; p.K = K; p.H = n_hidden; p.n_rows = n_rows; p.mode = sample_mode; p.seed = seed;
  const long long tiles = (long long)((M + RT - 1) / RT) * ((N + RT - 1) / RT);
  if (tiles > 0x7fffffffLL) return SFM_ERR_SHAPE;
  dim3 grid((unsigned)tiles), block(256);
  if (down) SFM_LAUNCH((rbm_prob_kernel<true>), grid, block, 0, (hipStream_t)stream, p);
  else SFM_LAUNCH((rbm_prob_kernel<false>), grid, block, 0, (hipStream_t)stream, p);
  return SFM_OK;
}

extern "C" int sfm_rbm_update(const float* data, const int* rows, const float* ph, const float* nv, const float* nh, float* W,
                              float* v_bias, float* h_bias, double* err_partial, int B, int n_visible, int n_hidden, int n_rows,
                              long long ldv, float lr, void* stream) {
  if (!data || !ph || !nv || !nh || !W || !v_bias || !h_bias || !err_partial) return SFM_ERR_ARG;
  if (!(lr == lr)) return SFM_ERR_ARG;
  if (B < 1 || B > SFM_RBM_MAX_BATCH || n_rows < 1 || !rbm_units_ok(n_visible, n_hidden)) return SFM_ERR_SHAPE;
  if (ldv < n_visible || (!rows && B > n_rows)) return SFM_ERR_SHAPE;
  RbmUpdateParams p;
  p.data = data; p.rows = rows; p.ph = ph; p.nv = nv; p.nh = nh; p.W = W; p.v_bias = v_bias; p.h_bias = h_bias;
  p.err_partial = err_partial; p.ldv = ldv; p.B = B; p.V = n_visible; p.H = n_hidden; p.n_rows = n_rows; p.lr = lr;
  dim3 grid((unsigned)(((n_visible + RT - 1) / RT) * ((n_hidden + RT - 1) / RT))), block(256);
  SFM_LAUNCH(rbm_update_kernel, grid, block, 0, (hipStream_t)stream, p);
  return SFM_OK;
}

extern "C" int sfm_rbm_fold_error(const double* partial, double* out, int n_steps, int n_tiles, int num_samples, int batch_size,
                                  int n_visible, void* stream) {
  if (!partial || !out) return SFM_ERR_ARG;
  if (n_steps < 1 || n_tiles < 1 || num_samples < 1 || batch_size < 1 || n_visible < 1) return SFM_ERR_SHAPE;
  if ((long long)n_tiles != (n_visible + RT - 1) / RT) return SFM_ERR_SHAPE;
  if ((long long)n_steps != ((long long)num_samples + batch_size - 1) / batch_size) return SFM_ERR_SHAPE;
  SFM_LAUNCH(rbm_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, out, n_steps, n_tiles, num_samples, batch_size,
             n_visible);
  return SFM_OK;
}
