// The PSO search of OPT-PCIRM's middle step (masks/opt_pcirm.py:101-202, optimizer/pso.py) with the STOI fallback
// (evaluation/stoi.py:53-99) as fitness, for a batch of utterances: one swarm of N particles per utterance.
//
// The fitness of a candidate middle value x is a function of two fixed signals.  quantize_pcirm puts x into exactly the units
// of step 2 (M >= 3), so the channel mean of mask frame n is a[n] + x b[n]; the overlap-add of the mask frames divided by
// max(weights, 1) is a per-sample gain ga[t] + x gb[t]; enhanced(x) = ya + x yb with ya = noisy ga, yb = noisy gb, and - the DFT
// being linear - STOI frame k of enhanced(x) has the spectrum A_k + x B_k.  What is computed once per search:
//   pso_frame_coef_kernel   pcirm [B, C, T] -> a, b [B, T] (fp64): integer bucket counts, membership decided in double as
//                           quant_rule of masks.hip decides it, the assigned values rounded to fp32 as the mask array holds them
//   pso_split_kernel        noisy, clean [B, Lmax] -> ya, yb, clean packed back to back (fp32) and one fp64 partial of
//                           {sum ya^2, sum ya yb, sum yb^2, sum clean^2} per SFM_PSO_CHUNK samples; pso_moments_kernel folds the
//                           chunks of each utterance in index order (the convention of the SNR mix)
// and per round of the search (max_iter + 1 rounds, no host synchronisation):
//   pso_fitness_kernel      grid (chunk of SFM_PSO_FRAMES STOI frames, utterance): a wave keeps one frame's |C|, A, B in registers and
//                           loops over the N positions; evaluation/stoi.py:84-95 per frame and particle in fp64; the frames of
//                           a chunk are added in frame order: one fp64 partial per (utterance, chunk, particle)
//   pso_step_kernel         one workgroup per swarm, one thread per particle: folds the chunks in order, then optimizer/pso.py
//                           :92-110 (round 0) or :114-179 (one iteration) in fp64, bit for bit as numpy computes them: this file
//                           is compiled with -ffp-contract=off (build.py), sums over the particles follow numpy's pairwise rule
//   pso_quantize_kernel     the final mask, each utterance quantised with its own middle value
// No atomics anywhere: the same bits from run to run, and an utterance gets the same bits alone and in any batch.
// The search on the STOI / ESTOI of Taal et al. uses the first two and the last two kernels as they are; its fitness
// (pso_fitness_taal_kernel) stands in stoi.hip beside the segment arithmetic it shares with the measure, which is compiled with
// fused multiply-adds - this file is not - and hands pso_step_kernel its values as `fit_in`.
#include "sfm_common.h"
#include <math.h>

static_assert(SFM_PSO_CHUNK == 16 * 256, "a workgroup's chunk of the split: 16 samples per thread");
static_assert(SFM_PSO_FRAMES == 2 * 4, "STOI frames per workgroup of the fitness: 2 per wave");
static_assert(SFM_PSO_MAX_BINS == 16 * 64, "pso_fitness_kernel<16> holds 16 bins per lane");

// index of the step that holds x (the reference's loop: a later step overrides an earlier one), -1 where none does
static __device__ __forceinline__ int pso_bucket(float x, const double* __restrict__ table, int M) {
  const double v = (double)x;
  int k = -1;
  for (int m = 0; m < M; ++m)
    if (v >= table[m] && v < table[m + 1]) k = m;
  if (v >= table[M]) k = M - 1;
  return k;
}

__global__ __launch_bounds__(256) void pso_frame_coef_kernel(const float* __restrict__ pcirm, const double* __restrict__ table,
                                                             double* __restrict__ a, double* __restrict__ b, int C, int T, int M) {
  const int t = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
  if (t >= T) return;
  int cnt[SFM_QUANT_MAX_STEPS];
#pragma unroll
  for (int m = 0; m < SFM_QUANT_MAX_STEPS; ++m) cnt[m] = 0;
  const float* col = pcirm + (long long)u * C * T + t;
  for (int c = 0; c < C; ++c) {
    const int k = pso_bucket(col[(long long)c * T], table, M);
#pragma unroll
    for (int m = 0; m < SFM_QUANT_MAX_STEPS; ++m) cnt[m] += (k == m) ? 1 : 0;
  }
  const int mid = M >= 3 ? 1 : -1;       // M < 3: the middle value is unused, step 2 keeps its own value
  double s = 0.0;
  int nb = 0;
#pragma unroll
  for (int m = 0; m < SFM_QUANT_MAX_STEPS; ++m) {
    if (m >= M) continue;
    if (m == mid) nb = cnt[m];
    else s += (double)cnt[m] * (double)(float)table[M + 1 + m];
  }
  a[(long long)u * T + t] = s / (double)C;
  b[(long long)u * T + t] = (double)nb / (double)C;
}

static __device__ __forceinline__ int pso_len(const int* __restrict__ lengths, const int* __restrict__ samp_off, int u, int Lmax) {
  int len = lengths[u];
  const int room = samp_off[u + 1] - samp_off[u];
  len = len > Lmax ? Lmax : len;
  len = len > room ? room : len;
  return len < 0 ? 0 : len;
}

__global__ __launch_bounds__(256) void pso_split_kernel(const float* __restrict__ noisy, const float* __restrict__ clean,
                                                        const int* __restrict__ lengths, const int* __restrict__ samp_off,
                                                        const double* __restrict__ a, const double* __restrict__ b,
                                                        float* __restrict__ ya, float* __restrict__ yb, float* __restrict__ cp,
                                                        double* __restrict__ part, int Lmax, int T, int frame, int hop) {
  __shared__ double red[4][4];
  const int u = blockIdx.y, tid = threadIdx.x;
  const int len = pso_len(lengths, samp_off, u, Lmax);
  const int j0 = blockIdx.x * SFM_PSO_CHUNK;
  int j1 = j0 + SFM_PSO_CHUNK;
  if (j1 > len) j1 = len;
  const long long src = (long long)u * Lmax, dst = samp_off[u];
  const double* au = a + (long long)u * T;
  const double* bu = b + (long long)u * T;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = j0 + tid; t < j1; t += 256) {
    // mask frame n covers the samples [n hop, min(n hop + frame, len)), n < T: added in frame order, divided by max(count, 1)
    int n1 = t / hop;
    int n0 = t - frame + 1 <= 0 ? 0 : (t - frame + hop) / hop;
    if (n1 > T - 1) n1 = T - 1;
    double ga = 0.0, gb = 0.0;
    for (int n = n0; n <= n1; ++n) {
      ga += au[n];
      gb += bu[n];
    }
    const double w = n1 >= n0 ? (double)(n1 - n0 + 1) : 1.0;
    const double x = (double)noisy[src + t];
    const float fa = (float)(x * ga / w), fb = (float)(x * gb / w), fc = clean[src + t];
    ya[dst + t] = fa;
    yb[dst + t] = fb;
    cp[dst + t] = fc;
    s[0] += (double)fa * (double)fa;
    s[1] += (double)fa * (double)fb;
    s[2] += (double)fb * (double)fb;
    s[3] += (double)fc * (double)fc;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[q] = wave_sum_d(s[q]);
    if ((tid & 63) == 0) red[q][tid >> 6] = s[q];
  }
  __syncthreads();
  if (tid < 4) part[((long long)u * gridDim.x + blockIdx.x) * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// utterance u's NC chunk partials in index order -> S[u] = {sum ya^2, sum ya yb, sum yb^2, sum clean^2}
__global__ __launch_bounds__(256) void pso_moments_kernel(const double* __restrict__ part, double* __restrict__ S, int B, int NC) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * B) return;
  const int u = i >> 2, q = i & 3;
  double s = 0.0;
  for (int c = 0; c < NC; ++c) s += part[((long long)u * NC + c) * 4 + q];
  S[i] = s;
}

// NB: bins per lane, F <= 64 NB
template <int NB>
__global__ __launch_bounds__(256) void pso_fitness_kernel(const float* __restrict__ cr, const float* __restrict__ ci,
                                                          const float* __restrict__ ar, const float* __restrict__ ai,
                                                          const float* __restrict__ br, const float* __restrict__ bi,
                                                          const int* __restrict__ frame_off, const int* __restrict__ lengths,
                                                          const double* __restrict__ S, const double* __restrict__ pos,
                                                          const int* __restrict__ stopped, double* __restrict__ partial, int N,
                                                          int F, int NC) {
  __shared__ double corr[SFM_PSO_FRAMES][SFM_PSO_MAX_PARTICLES];
  __shared__ double xs[SFM_PSO_MAX_PARTICLES], kes[SFM_PSO_MAX_PARTICLES];
  const int u = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (stopped[u]) return;
  const int f0 = frame_off[u], nf = frame_off[u + 1] - f0, k0 = c * SFM_PSO_FRAMES;
  if (k0 >= nf) return;
  const int kn = nf - k0 < SFM_PSO_FRAMES ? nf - k0 : SFM_PSO_FRAMES;
  const double Ls = (double)(lengths[u] < 1 ? 1 : lengths[u]);
  const double kc = 1.0 / (sqrt(S[4 * u + 3] / Ls) + 1e-10);                 // evaluation/stoi.py:66
  if (tid < N) {
    const double x = (double)(float)pos[(long long)u * N + tid];             // the mask array is float32
    double msq = (S[4 * u] + 2.0 * x * S[4 * u + 1] + x * x * S[4 * u + 2]) / Ls;
    msq = msq > 0.0 ? msq : 0.0;
    xs[tid] = x;
    kes[tid] = 1.0 / (sqrt(msq) + 1e-10);                                    // :67
  }
  __syncthreads();
  for (int j = wave; j < kn; j += 4) {
    const long long row = (long long)(f0 + k0 + j) * F;
    double cm[NB];
    float a0[NB], a1[NB], b0[NB], b1[NB];
    double A = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int f = lane + 64 * i;
      const bool in = f < F;
      const double c0 = in ? (double)cr[row + f] : 0.0, c1 = in ? (double)ci[row + f] : 0.0;
      a0[i] = in ? ar[row + f] : 0.f;
      a1[i] = in ? ai[row + f] : 0.f;
      b0[i] = in ? br[row + f] : 0.f;
      b1[i] = in ? bi[row + f] : 0.f;
      cm[i] = sqrt(c0 * c0 + c1 * c1) * kc;
      A += cm[i] * cm[i];
    }
    A = wave_sum_d(A);
    const double clean_energy = sqrt(A + 1e-10);                             // :88
    for (int p = 0; p < N; ++p) {
      const double x = xs[p], ke = kes[p];
      double Bq = 0.0, Cx = 0.0;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const double e0 = (double)a0[i] + x * (double)b0[i], e1 = (double)a1[i] + x * (double)b1[i];
        const double em = sqrt(e0 * e0 + e1 * e1) * ke;
        Bq += em * em;
        Cx += cm[i] * em;
      }
      Bq = wave_sum_d(Bq);
      Cx = wave_sum_d(Cx);
      const double k = clean_energy / (sqrt(Bq) + 1e-10);                    // :89, enh_norm = enh_spec k
      const double v = (k * Cx) / (sqrt(A * (k * k * Bq)) + 1e-10);          // :92-94
      if (lane == 0) corr[j][p] = fmin(fmax(v, -1.0), 1.0);
    }
  }
  __syncthreads();
  if (tid < N) {
    double s = 0.0;
    for (int j = 0; j < kn; ++j) s += corr[j][tid];
    partial[((long long)u * NC + c) * N + tid] = s;
  }
}

// np.add.reduce of a contiguous float64 vector: pairwise, 8 accumulators below 128 elements (numpy's DOUBLE_pairwise_sum)
static __device__ double pso_np_sum(const double* v, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += v[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = v[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += v[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return pso_np_sum(v, n2) + pso_np_sum(v + n2, n - n2);
}

static __device__ __forceinline__ bool pso_better(double x, double y, int maximize) { return maximize ? x > y : x < y; }

// params: {w, c1, c2, lb, ub}.  hist row `it` of swarm u: {gbest fitness, gbest position, mean fitness, position[N], fitness[N]}
__global__ __launch_bounds__(SFM_PSO_MAX_PARTICLES) void pso_step_kernel(const double* __restrict__ partial,
                                                                         const double* __restrict__ fit_in,
                                                             const int* __restrict__ frame_off, const double* __restrict__ draws,
                                                             const double* __restrict__ params, double* __restrict__ pos,
                                                             double* __restrict__ vel, double* __restrict__ pbest_pos,
                                                             double* __restrict__ pbest_fit, double* __restrict__ gbest,
                                                             double* __restrict__ hist, int* __restrict__ iters,
                                                             int* __restrict__ stopped, int N, int NC, int it, int max_iter,
                                                             int maximize) {
  __shared__ double s_fit[SFM_PSO_MAX_PARTICLES], s_pos[SFM_PSO_MAX_PARTICLES], s_pbf[SFM_PSO_MAX_PARTICLES],
      s_pbp[SFM_PSO_MAX_PARTICLES], s_dev[SFM_PSO_MAX_PARTICLES];
  __shared__ double s_g;
  __shared__ int s_done;
  const int u = blockIdx.x, p = threadIdx.x;
  if (stopped[u]) return;
  const bool live = p < N;
  const long long q = (long long)u * N + p;
  double x = 0.0, v = 0.0, fit = 0.0, pbp = 0.0, pbf = 0.0;
  if (live) {
    if (fit_in) {
      fit = fit_in[q];
    } else {
      const int nf = frame_off[u + 1] - frame_off[u];
      if (nf > 0) {
        int nc = (nf + SFM_PSO_FRAMES - 1) / SFM_PSO_FRAMES;
        if (nc > NC) nc = NC;
        double s = 0.0;
        for (int c = 0; c < nc; ++c) s += partial[((long long)u * NC + c) * N + p];
        s = s / (double)nf;                                                  // evaluation/stoi.py:98-99
        fit = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
      }
    }
    x = pos[q];
    v = vel[q];
    if (it == 0) {
      pbp = x;
      pbf = fit;
    } else {
      pbp = pbest_pos[q];
      pbf = pbest_fit[q];
      if (pso_better(fit, pbf, maximize)) {
        pbf = fit;
        pbp = x;
      }
    }
    s_fit[p] = fit;
    s_pos[p] = x;
    s_pbf[p] = pbf;
    s_pbp[p] = pbp;
  }
  __syncthreads();
  double* row = hist + ((long long)u * (max_iter + 1) + it) * (3 + 2 * N);
  if (p == 0) {
    double gp, gf;
    int best = 0;
    if (it == 0) {
      for (int i = 1; i < N; ++i)
        if (pso_better(s_fit[i], s_fit[best], maximize)) best = i;
      gp = s_pos[best];
      gf = s_fit[best];
    } else {
      gp = gbest[2 * u];
      gf = gbest[2 * u + 1];
      for (int i = 1; i < N; ++i)
        if (pso_better(s_pbf[i], s_pbf[best], maximize)) best = i;
      if (pso_better(s_pbf[best], gf, maximize)) {
        gf = s_pbf[best];
        gp = s_pbp[best];
      }
    }
    gbest[2 * u] = gp;
    gbest[2 * u + 1] = gf;
    row[0] = gf;
    row[1] = gp;
    row[2] = pso_np_sum(s_fit, N) / (double)N;
    int stop = 0;
    if (it > 0) {                                                            // np.std(positions) < 1e-6, two-pass
      const double mean = pso_np_sum(s_pos, N) / (double)N;
      for (int i = 0; i < N; ++i) {
        const double d = s_pos[i] - mean;
        s_dev[i] = d * d;
      }
      stop = sqrt(pso_np_sum(s_dev, N) / (double)N) < 1e-6;
    }
    iters[u] = it;
    if (stop) stopped[u] = 1;
    s_done = stop || it >= max_iter;
    s_g = gp;
  }
  __syncthreads();
  if (!live) return;
  row[3 + p] = x;
  row[3 + N + p] = fit;
  pbest_pos[q] = pbp;
  pbest_fit[q] = pbf;
  if (s_done) return;
  const double w = params[0], c1 = params[1], c2 = params[2], lb = params[3], ub = params[4];
  const double* r = draws + (long long)u * (2 * N + 2LL * N * max_iter) + 2 * N + 2 * ((long long)it * N + p);
  const double cognitive = (c1 * r[0]) * (pbp - x), social = (c2 * r[1]) * (s_g - x);
  v = (w * v + cognitive) + social;
  const double max_v = (ub - lb) * 0.5;
  v = v < -max_v ? -max_v : (v > max_v ? max_v : v);
  x = x + v;
  if (x < lb) {
    x = lb;
    v = fabs(v) * 0.5;
  } else if (x > ub) {
    x = ub;
    v = -fabs(v) * 0.5;
  }
  pos[q] = x;
  vel[q] = v;
}

__global__ __launch_bounds__(256) void pso_quantize_kernel(const float* __restrict__ pcirm, const double* __restrict__ table,
                                                           const double* __restrict__ middle, float* __restrict__ out,
                                                           long long CT, int M) {
  const int u = blockIdx.y;
  const float mid = (float)middle[u];
  const float* in = pcirm + (long long)u * CT;
  float* o = out + (long long)u * CT;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < CT; i += (long long)gridDim.x * 256) {
    const int k = pso_bucket(in[i], table, M);
    o[i] = k < 0 ? 0.f : ((k == 1 && M >= 3) ? mid : (float)table[M + 1 + k]);
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
static int pso_steps(int M) { return M < 2 || M > SFM_QUANT_MAX_STEPS ? SFM_ERR_SHAPE : SFM_OK; }

extern "C" int sfm_pso_frame_coef(const float* pcirm, const double* table, double* a, double* b, int B, int C, int T, int M,
                                  void* stream) {
  if (!pcirm || !table || !a || !b) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || C <= 0 || T <= 0 || pso_steps(M) != SFM_OK) return SFM_ERR_SHAPE;
  if ((long long)B * C * T > 2147483647LL) return SFM_ERR_SHAPE;
  SFM_LAUNCH(pso_frame_coef_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, pcirm, table,
             a, b, C, T, M);
  return SFM_OK;
}

static int pso_chunks(int Lmax) { return (Lmax + SFM_PSO_CHUNK - 1) / SFM_PSO_CHUNK; }
// ws of sfm_pso_split: the four sums' partials per utterance and chunk
extern "C" long long sfm_pso_split_ws_doubles(int B, int Lmax) { return B > 0 && Lmax > 0 ? 4LL * B * pso_chunks(Lmax) : 0; }

extern "C" int sfm_pso_split(const float* noisy, const float* clean, const int* lengths, const int* samp_off, const double* a,
                             const double* b, float* ya, float* yb, float* clean_packed, double* ws, double* S, int B, int Lmax,
                             int T, int frame, int hop, void* stream) {
  if (!noisy || !clean || !lengths || !samp_off || !a || !b || !ya || !yb || !clean_packed || !ws || !S) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || Lmax <= 0 || T <= 0 || hop <= 0 || frame < hop) return SFM_ERR_SHAPE;
  if ((long long)B * Lmax > 2147483647LL) return SFM_ERR_SHAPE;
  const int NC = pso_chunks(Lmax);
  hipStream_t st = (hipStream_t)stream;
  SFM_LAUNCH(pso_split_kernel, dim3((unsigned)NC, (unsigned)B), dim3(256), 0, st, noisy, clean, lengths, samp_off, a, b, ya, yb,
             clean_packed, ws, Lmax, T, frame, hop);
  SFM_LAUNCH(pso_moments_kernel, dim3((unsigned)((4 * B + 255) / 256)), dim3(256), 0, st, ws, S, B, NC);
  return SFM_OK;
}

static int pso_swarm(int B, int N) { return B <= 0 || B > 65535 || N < 1 || N > SFM_PSO_MAX_PARTICLES ? SFM_ERR_SHAPE : SFM_OK; }

extern "C" int sfm_pso_fitness(const float* cr, const float* ci, const float* ar, const float* ai, const float* br, const float* bi,
                               const int* frame_off, const int* lengths, const double* S, const double* pos, const int* stopped,
                               double* partial, int B, int N, int F, int NC, void* stream) {
  if (!cr || !ci || !ar || !ai || !br || !bi || !frame_off || !lengths || !S || !pos || !stopped || !partial) return SFM_ERR_ARG;
  if (pso_swarm(B, N) != SFM_OK || F <= 0 || F > SFM_PSO_MAX_BINS || NC <= 0) return SFM_ERR_SHAPE;
  const dim3 grid((unsigned)NC, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (F <= 128)
    SFM_LAUNCH((pso_fitness_kernel<2>), grid, dim3(256), 0, st, cr, ci, ar, ai, br, bi, frame_off, lengths, S, pos, stopped, partial,
               N, F, NC);
  else if (F <= 256)
    SFM_LAUNCH((pso_fitness_kernel<4>), grid, dim3(256), 0, st, cr, ci, ar, ai, br, bi, frame_off, lengths, S, pos, stopped, partial,
               N, F, NC);
  else
    SFM_LAUNCH((pso_fitness_kernel<16>), grid, dim3(256), 0, st, cr, ci, ar, ai, br, bi, frame_off, lengths, S, pos, stopped,
               partial, N, F, NC);
  return SFM_OK;
}

extern "C" int sfm_pso_step(const double* partial, const double* fitness, const int* frame_off, const double* draws,
                            const double* params, double* pos, double* vel, double* pbest_pos, double* pbest_fit, double* gbest,
                            double* hist, int* iters, int* stopped, int B, int N, int NC, int it, int max_iter, int maximize,
                            void* stream) {
  if (!draws || !params || !pos || !vel || !pbest_pos || !pbest_fit || !gbest || !hist || !iters || !stopped) return SFM_ERR_ARG;
  if ((partial != nullptr) == (fitness != nullptr) || (partial && !frame_off)) return SFM_ERR_ARG;
  if (pso_swarm(B, N) != SFM_OK || max_iter < 1 || it < 0 || it > max_iter || (partial && NC <= 0)) return SFM_ERR_SHAPE;
  SFM_LAUNCH(pso_step_kernel, dim3((unsigned)B), dim3(SFM_PSO_MAX_PARTICLES), 0, (hipStream_t)stream, partial, fitness, frame_off,
             draws, params, pos, vel, pbest_pos, pbest_fit, gbest, hist, iters, stopped, N, NC, it, max_iter, maximize ? 1 : 0);
  return SFM_OK;
}

extern "C" int sfm_pso_quantize(const float* pcirm, const double* table, const double* middle, float* out, int B, long long CT,
                                int M, void* stream) {
  if (!pcirm || !table || !middle || !out) return SFM_ERR_ARG;
  if (B <= 0 || B > 65535 || CT <= 0 || pso_steps(M) != SFM_OK || (long long)B * CT > 2147483647LL) return SFM_ERR_SHAPE;
  long long nb = (CT + 255) / 256;
  if (nb > 1024) nb = 1024;
  SFM_LAUNCH(pso_quantize_kernel, dim3((unsigned)nb, (unsigned)B), dim3(256), 0, (hipStream_t)stream, pcirm, table, middle, out, CT,
             M);
  return SFM_OK;
}
