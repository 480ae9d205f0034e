// Curriculum batches (stages 1 and 2): the SNR mix of training/conformer_pipeline.py:142-150 over a batch, and the soft / hard mask
// targets of masks/{irm,pcirm,opt_pcirm}.py.  Everything here is memory-bound: flat ranges, 16-byte accesses between a scalar
// head and tail, no atomics (the powers of the mix go through one fp64 partial per workgroup and an ordered fold).
//
// elementwise  one skeleton (mask_ew_kernel) over n contiguous floats per plane; an Op names its planes and the per-element rule:
//   IrmOp      (c^2 / (c^2 + n^2 + eps))^p, sqrtf for p = 0.5, clipped to [0, 1]                       masks/irm.py:17-39
//   CorrOp     |a b| / (sqrt(a^2 + eps) sqrt(b^2 + eps)) for (noisy, clean) and (noisy, noise)          masks/pcirm.py:49-57, 70-72
//   PcirmOp    rho_s (c |cos phi1|)^2 / (the same + rho_n (n |cos phi2|)^2 + eps)                       masks/pcirm.py:122-131
//   QuantOp    the step of `table` whose [boundary m, boundary m + 1) holds x, compared in double      masks/opt_pcirm.py:79-101
//   CurrOp     Y = C + s[b] N and the mask target from C, s N, Y; the cosines of the phase differences are Re(C conj Y) / (|C| |Y|)
// mix          mix_power_kernel: fp64 sums of clean^2 and noise^2 over fixed SFM_MIX_CHUNK-sample chunks of each utterance;
//              mix_scale_kernel: ONE workgroup folds the chunks of each utterance in index order and writes scale;
//              mix_apply_kernel: noisy = clean + scale * noise (0 at and beyond the utterance's length), and on request the
//              unscaled noise row the utterance was mixed with (the operand of the noise STFT).
// packed set   training.WaveformSet keeps its clean utterances back to back: mix_power_varlen_kernel / mix_scale_varlen_kernel are
//              the two mix kernels above on packed[off[u] .. off[u + 1]), and wave_batch_kernel gathers the rows of an index list,
//              mixes them and writes the step's (noisy, clean) pair in one launch.
#include "sfm_common.h"
#include <math.h>

static_assert(SFM_MIX_CHUNK == 16 * 256, "a workgroup's chunk: 16 samples per thread");

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static __device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // (a NaN stays one: np.clip)

// ---- the elementwise skeleton ------------------------------------------------------------------------------------------------
// Op: NI input planes `in`, NO output planes `out` (a NULL output is skipped), Ctx begin(i) once per thread-iteration and
// f(x, y, ctx, k) for element i + k of it (k = 0 in the scalar head / tail).
template <class Op>
static __device__ __forceinline__ void ew_one(const Op& op, long long i) {
  float x[Op::NI], y[Op::NO];
#pragma unroll
  for (int a = 0; a < Op::NI; ++a) x[a] = op.in[a][i];
  const auto ctx = op.begin(i);
  op.f(x, y, ctx, 0);
#pragma unroll
  for (int o = 0; o < Op::NO; ++o)
    if (op.out[o]) op.out[o][i] = y[o];
}
template <class Op>
__global__ __launch_bounds__(256) void mask_ew_kernel(const Op op, long long n, int vec) {
  const long long stride = (long long)gridDim.x * 256, gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nq = vec ? n >> 2 : 0;
  for (long long q = gid; q < nq; q += stride) {
    const long long i = q << 2;
    f32x4 v[Op::NI], w[Op::NO];
#pragma unroll
    for (int a = 0; a < Op::NI; ++a) v[a] = *reinterpret_cast<const f32x4*>(op.in[a] + i);
    const auto ctx = op.begin(i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x[Op::NI], y[Op::NO];
#pragma unroll
      for (int a = 0; a < Op::NI; ++a) x[a] = v[a][k];
      op.f(x, y, ctx, k);
#pragma unroll
      for (int o = 0; o < Op::NO; ++o) w[o][k] = y[o];
    }
#pragma unroll
    for (int o = 0; o < Op::NO; ++o)
      if (op.out[o]) *reinterpret_cast<f32x4*>(op.out[o] + i) = w[o];
  }
  for (long long i = (nq << 2) + gid; i < n; i += stride) ew_one(op, i);
}

template <class Op>
static int ew_launch(const Op& op, long long n, void* stream) {
  int vec = 1;
  for (int a = 0; a < Op::NI; ++a) vec &= al16(op.in[a]);
  for (int o = 0; o < Op::NO; ++o) vec &= al16(op.out[o]);
  long long nb = (((n + 3) >> 2) + 255) / 256;
  if (nb > 4096) nb = 4096;
  SFM_LAUNCH((mask_ew_kernel<Op>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, op, n, vec);
  return SFM_OK;
}

struct NoCtx {};

static __device__ __forceinline__ float irm_rule(float c2, float n2, float p, float eps, bool root) {
  const float r = c2 / (c2 + n2 + eps);
  return clip01(root ? sqrtf(r) : powf(r, p));
}

struct IrmOp {
  static constexpr int NI = 2, NO = 1;
  const float* in[NI];
  float* out[NO];
  float p, eps;
  int root;
  __device__ __forceinline__ NoCtx begin(long long) const { return NoCtx(); }
  __device__ __forceinline__ void f(const float (&x)[NI], float (&y)[NO], NoCtx, int) const {
    y[0] = irm_rule(x[0] * x[0], x[1] * x[1], p, eps, root != 0);
  }
};

static __device__ __forceinline__ float corr_rule(float a, float b, float eps) {
  return clip01(fabsf(a * b / (sqrtf(a * a + eps) * sqrtf(b * b + eps))));
}

struct CorrOp {
  static constexpr int NI = 3, NO = 2;
  const float* in[NI];                   // noisy, clean, noise
  float* out[NO];                        // rho_s, rho_n
  float eps;
  __device__ __forceinline__ NoCtx begin(long long) const { return NoCtx(); }
  __device__ __forceinline__ void f(const float (&x)[NI], float (&y)[NO], NoCtx, int) const {
    y[0] = corr_rule(x[0], x[1], eps);
    y[1] = corr_rule(x[0], x[2], eps);
  }
};

struct PcirmOp {
  static constexpr int NI = 6, NO = 1;
  const float* in[NI];                   // clean_mag, noise_mag, rho_s, rho_n, phi1, phi2
  float* out[NO];
  float eps;
  __device__ __forceinline__ NoCtx begin(long long) const { return NoCtx(); }
  __device__ __forceinline__ void f(const float (&x)[NI], float (&y)[NO], NoCtx, int) const {
    const float cs = fabsf(x[0]) * fabsf(cosf(x[4])), cn = fabsf(x[1]) * fabsf(cosf(x[5]));
    const float sp = x[2] * (cs * cs), no = x[3] * (cn * cn);
    y[0] = clip01(sp / (sp + no + eps));
  }
};

// table: M + 1 boundaries, then M values (doubles).  The reference's loop, a later step overriding an earlier one; what no
// step holds (a NaN, a negative value) stays 0.
static __device__ __forceinline__ float quant_rule(float x, const double* __restrict__ table, int M) {
  const double v = (double)x;
  double q = 0.0;
  for (int m = 0; m < M; ++m)
    if (v >= table[m] && v < table[m + 1]) q = table[M + 1 + m];
  if (v >= table[M]) q = table[2 * M];
  return (float)q;
}

struct QuantOp {
  static constexpr int NI = 1, NO = 1;
  const float* in[NI];
  float* out[NO];
  const double* table;
  int M;
  __device__ __forceinline__ NoCtx begin(long long) const { return NoCtx(); }
  __device__ __forceinline__ void f(const float (&x)[NI], float (&y)[NO], NoCtx, int) const { y[0] = quant_rule(x[0], table, M); }
};

// kind (SFM_MASK_*): NONE spectra only, IRM, PCIRM, OPT_PCIRM (the PCIRM, quantised by `table`)
struct CurrCtx {
  float s0, s1;                          // scale of the utterance of element i, and of the next one
  int left;                              // elements of this utterance from i on
};
struct CurrOp {
  static constexpr int NI = 4, NO = 3;
  const float* in[NI];                   // Cr, Ci, Nr, Ni
  float* out[NO];                        // Yr, Yi, mask
  const float* scale;
  const double* table;
  int B, TF, kind, M, root;
  float p, eps;
  __device__ __forceinline__ CurrCtx begin(long long i) const {
    const unsigned b = (unsigned)i / (unsigned)TF;                       // (n <= 2^31 - 1: checked by the launcher)
    CurrCtx c;
    c.s0 = scale[b];
    c.s1 = scale[b + 1 < (unsigned)B ? b + 1 : b];
    c.left = (int)((b + 1) * (unsigned)TF - (unsigned)i);
    return c;
  }
  __device__ __forceinline__ void f(const float (&x)[NI], float (&y)[NO], CurrCtx c, int k) const {
    const float s = k < c.left ? c.s0 : c.s1;                            // a quad crosses at most one boundary (TF >= 4 when vec)
    const float cr = x[0], ci = x[1], nr = s * x[2], ni = s * x[3];
    const float yr = cr + nr, yi = ci + ni;
    y[0] = yr;
    y[1] = yi;
    if (kind == SFM_MASK_NONE) {
      y[2] = 0.f;
      return;
    }
    const float c2 = cr * cr + ci * ci, n2 = nr * nr + ni * ni;
    if (kind == SFM_MASK_IRM) {
      y[2] = irm_rule(c2, n2, p, eps, root != 0);
      return;
    }
    // PCIRM on |C|, |sN|, |Y| and the phase differences to Y.  rho_s = |Y||C| / (sqrt(|Y|^2 + eps) sqrt(|C|^2 + eps)) under one
    // root; (|C| cos phi1)^2 = Re(C conj Y)^2 / |Y|^2, no angle taken.  A zero magnitude counts as phase 0 (np.angle): C = 0
    // leaves Re(C conj Y) = 0 and Y = 0 leaves rho = 0, so either way the component is 0, as it is there.
    const float y2 = yr * yr + yi * yi;
    float sp = 0.f, no = 0.f;
    if (y2 > 0.f) {
      const float d1 = cr * yr + ci * yi, d2 = nr * yr + ni * yi, ry = 1.f / y2, ye = y2 + eps;
      sp = sqrtf((y2 * c2) / (ye * (c2 + eps))) * (d1 * d1 * ry);
      no = sqrtf((y2 * n2) / (ye * (n2 + eps))) * (d2 * d2 * ry);
    }
    const float m = clip01(sp / (sp + no + eps));
    y[2] = kind == SFM_MASK_OPT_PCIRM ? quant_rule(m, table, M) : m;
  }
};

// ---- the mix ------------------------------------------------------------------------------------------------------------------
struct MixRow {
  const float* noise;                    // the utterance's noise, Ln samples (Ln = 0: none)
  int Ln, len;
};
static __device__ __forceinline__ MixRow mix_row(const float* __restrict__ bank, const int* __restrict__ off,
                                                 const int* __restrict__ ids, const int* __restrict__ lengths, int b, int L,
                                                 int n_noise) {
  int id = ids[b];
  id = id < 0 ? 0 : (id >= n_noise ? n_noise - 1 : id);
  int len = lengths ? lengths[b] : L;
  len = len < 0 ? 0 : (len > L ? L : len);
  MixRow r;
  r.noise = bank + off[id];
  r.Ln = off[id + 1] - off[id];
  if (r.Ln < 0) r.Ln = 0;
  r.len = r.Ln > 0 ? len : 0;            // (an empty noise entry: nothing to mix, the row is written as zeros)
  return r;
}
// sample j of the tiled / cut noise: noise[j mod Ln]
static __device__ __forceinline__ int mix_wrap(int j, int Ln) { return j < Ln ? j : (int)((unsigned)j % (unsigned)Ln); }

// The samples [j0, j1) of row b of a [B, L] array whose first element is 16-byte aligned (vec): `head` scalars up to the
// first aligned one, nq quads, then the tail.  vec == 0: all scalars.
struct RowSplit {
  int head, nq, rest;
};
static __device__ __forceinline__ RowSplit row_split(long long first, int count, int vec) {
  RowSplit s;
  s.head = vec ? (int)((4 - (first & 3)) & 3) : count;
  if (s.head > count) s.head = count;
  s.nq = (count - s.head) >> 2;
  s.rest = count - s.head - 4 * s.nq;
  return s;
}

// one workgroup's (clean^2, noise^2) partial: the samples [j0, j0 + SFM_MIX_CHUNK) below r.len of the utterance `row`, whose sample
// 0 is element `first` of a buffer that is 16-byte aligned when vec
static __device__ __forceinline__ void mix_power_chunk(const float* __restrict__ row, long long first, const MixRow r, int j0,
                                                       double* __restrict__ o, int vec) {
  __shared__ double red[8];
  const int tid = threadIdx.x;
  int j1 = j0 + SFM_MIX_CHUNK;
  if (j1 > r.len) j1 = r.len;
  double pc = 0.0, pn = 0.0;
  if (j1 > j0) {
    const RowSplit s = row_split(first + j0, j1 - j0, vec);
    for (int q = tid; q < s.nq; q += 256) {
      const int j = j0 + s.head + 4 * q;
      const f32x4 c = *reinterpret_cast<const f32x4*>(row + j);
      int w = mix_wrap(j, r.Ln);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double x = (double)c[k], z = (double)r.noise[w];
        pc += x * x;
        pn += z * z;
        w = w + 1 == r.Ln ? 0 : w + 1;
      }
    }
    for (int t = tid; t < s.head + s.rest; t += 256) {
      const int j = t < s.head ? j0 + t : j0 + 4 * s.nq + t;
      const double x = (double)row[j], z = (double)r.noise[mix_wrap(j, r.Ln)];
      pc += x * x;
      pn += z * z;
    }
  }
  pc = wave_sum_d(pc);
  pn = wave_sum_d(pn);
  if ((tid & 63) == 0) {
    red[tid >> 6] = pc;
    red[4 + (tid >> 6)] = pn;
  }
  __syncthreads();
  if (tid == 0) {
    o[0] = (red[0] + red[1]) + (red[2] + red[3]);
    o[1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

__global__ __launch_bounds__(256) void mix_power_kernel(const float* __restrict__ clean, const float* __restrict__ bank,
                                                        const int* __restrict__ off, const int* __restrict__ ids,
                                                        const int* __restrict__ lengths, double* __restrict__ part, int L,
                                                        int n_noise, int vec) {
  const int b = blockIdx.y;
  const MixRow r = mix_row(bank, off, ids, lengths, b, L, n_noise);
  mix_power_chunk(clean + (long long)b * L, (long long)b * L, r, blockIdx.x * SFM_MIX_CHUNK,
                  part + 2 * ((long long)b * gridDim.x + blockIdx.x), vec);
}

// The packed form: utterance u is packed[uoff[u] .. uoff[u + 1]) (offsets clamped to 0..total and to ascending), its length its own;
// the grid is the chunks of the longest utterance x the utterances, a chunk past an utterance's end writes a pair of zeros.
struct PackedRow {
  int start, len;
};
static __device__ __forceinline__ PackedRow packed_row(const int* __restrict__ uoff, int u, int total) {
  int s = uoff[u], e = uoff[u + 1];
  s = s < 0 ? 0 : (s > total ? total : s);
  e = e < s ? s : (e > total ? total : e);
  PackedRow p;
  p.start = s, p.len = e - s;
  return p;
}
static __device__ __forceinline__ MixRow packed_mix_row(const float* __restrict__ bank, const int* __restrict__ off, int id,
                                                        int len, int n_noise) {
  id = id < 0 ? 0 : (id >= n_noise ? n_noise - 1 : id);
  MixRow r;
  r.noise = bank + off[id];
  r.Ln = off[id + 1] - off[id];
  if (r.Ln < 0) r.Ln = 0;
  r.len = r.Ln > 0 ? len : 0;
  return r;
}

__global__ __launch_bounds__(256) void mix_power_varlen_kernel(const float* __restrict__ packed, const int* __restrict__ uoff,
                                                               const float* __restrict__ bank, const int* __restrict__ off,
                                                               const int* __restrict__ ids, double* __restrict__ part, int total,
                                                               int n_noise, int vec) {
  const int u = blockIdx.y;
  const PackedRow p = packed_row(uoff, u, total);
  const MixRow r = packed_mix_row(bank, off, ids[u], p.len, n_noise);
  mix_power_chunk(packed + p.start, p.start, r, blockIdx.x * SFM_MIX_CHUNK, part + 2 * ((long long)u * gridDim.x + blockIdx.x), vec);
}

// one workgroup: utterance b's NC chunk sums in index order, then scale = sqrt(Pc / (Pn 10^(snr / 10))), P = mean + 1e-10
__global__ __launch_bounds__(256) void mix_scale_kernel(const double* __restrict__ part, const float* __restrict__ snr_db,
                                                        const int* __restrict__ lengths, float* __restrict__ scale, int B, int L,
                                                        int NC) {
  for (int b = threadIdx.x; b < B; b += 256) {
    double sc = 0.0, sn = 0.0;
    const double* p = part + 2 * (long long)b * NC;
    for (int c = 0; c < NC; ++c) {
      sc += p[2 * c];
      sn += p[2 * c + 1];
    }
    int len = lengths ? lengths[b] : L;
    len = len < 1 ? 1 : (len > L ? L : len);
    const double pc = sc / (double)len + 1e-10, pn = sn / (double)len + 1e-10;
    scale[b] = (float)sqrt(pc / (pn * pow(10.0, (double)snr_db[b] / 10.0)));
  }
}

// the same fold and formula for packed utterances (a length below 1 counts as 1, as above)
__global__ __launch_bounds__(256) void mix_scale_varlen_kernel(const double* __restrict__ part, const float* __restrict__ snr_db,
                                                               const int* __restrict__ uoff, float* __restrict__ scale, int U,
                                                               int total, int NC) {
  for (int u = threadIdx.x; u < U; u += 256) {
    double sc = 0.0, sn = 0.0;
    const double* p = part + 2 * (long long)u * NC;
    for (int c = 0; c < NC; ++c) {
      sc += p[2 * c];
      sn += p[2 * c + 1];
    }
    int len = packed_row(uoff, u, total).len;
    len = len < 1 ? 1 : len;
    const double pc = sc / (double)len + 1e-10, pn = sn / (double)len + 1e-10;
    scale[u] = (float)sqrt(pc / (pn * pow(10.0, (double)snr_db[u] / 10.0)));
  }
}

__global__ __launch_bounds__(256) void mix_apply_kernel(const float* __restrict__ clean, const float* __restrict__ bank,
                                                        const int* __restrict__ off, const int* __restrict__ ids,
                                                        const int* __restrict__ lengths, const float* __restrict__ scale,
                                                        float* __restrict__ noisy, float* __restrict__ rows, int L, int n_noise,
                                                        int vec) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const MixRow r = mix_row(bank, off, ids, lengths, b, L, n_noise);
  const float sc = scale[b];
  const int j0 = blockIdx.x * SFM_MIX_CHUNK;
  int j1 = j0 + SFM_MIX_CHUNK;
  if (j1 > L) j1 = L;
  const long long base = (long long)b * L;
  const float* row = clean + base;
  float* out = noisy + base;
  float* nrow = rows ? rows + base : nullptr;
  const RowSplit s = row_split(base + j0, j1 - j0, vec);
  for (int q = tid; q < s.nq; q += 256) {
    const int j = j0 + s.head + 4 * q;
    f32x4 y = {0.f, 0.f, 0.f, 0.f}, z = {0.f, 0.f, 0.f, 0.f};
    if (j < r.len) {
      const f32x4 c = *reinterpret_cast<const f32x4*>(row + j);
      int w = mix_wrap(j, r.Ln);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (j + k < r.len) {
          z[k] = r.noise[w];
          y[k] = c[k] + sc * z[k];
        }
        w = w + 1 == r.Ln ? 0 : w + 1;
      }
    }
    *reinterpret_cast<f32x4*>(out + j) = y;
    if (nrow) *reinterpret_cast<f32x4*>(nrow + j) = z;
  }
  for (int t = tid; t < s.head + s.rest; t += 256) {
    const int j = t < s.head ? j0 + t : j0 + 4 * s.nq + t;
    float y = 0.f, z = 0.f;
    if (j < r.len) {
      z = r.noise[mix_wrap(j, r.Ln)];
      y = row[j] + sc * z;
    }
    out[j] = y;
    if (nrow) nrow[j] = z;
  }
}

// From an index list to a training step's two waveforms: out [2, B, L], plane 0 (blockIdx.z) = the mix of utterance index[b] of a
// packed set, plane 1 its clean samples, both 0 from the utterance's length on and in a row whose index is outside 0 .. U - 1
// (-1: dnn_layer_indexed's empty row).  The packed source row starts at any 4-byte boundary, so it is read with 4-byte-aligned
// 16-byte loads (global memory takes them); the stores are 16-byte ones where the OUTPUT row allows them (row_split).  A mixed
// sample is mix_apply_kernel's expression, so a row has that kernel's bits for the padded utterance.
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(256) void wave_batch_kernel(const float* __restrict__ packed, const int* __restrict__ uoff,
                                                         const float* __restrict__ bank, const int* __restrict__ off,
                                                         const int* __restrict__ ids, const float* __restrict__ scale,
                                                         const int* __restrict__ index, float* __restrict__ out, int B, int L, int U,
                                                         int total, int n_noise, int vec) {
  const int b = blockIdx.y, tid = threadIdx.x, mixed = blockIdx.z == 0;
  const int u = index[b];
  const float* row = packed;
  MixRow r;
  r.noise = bank, r.Ln = 0, r.len = 0;
  int len = 0;                           // samples of the utterance that the row holds
  float sc = 0.f;
  if (u >= 0 && u < U) {
    const PackedRow p = packed_row(uoff, u, total);
    len = p.len > L ? L : p.len;
    row = packed + p.start;
    if (mixed) {
      r = packed_mix_row(bank, off, ids[u], len, n_noise);
      sc = scale[u];
      len = r.len;                       // (an empty noise entry: zeros, as mix_apply_kernel writes them)
    }
  }
  const int j0 = blockIdx.x * SFM_MIX_CHUNK;
  int j1 = j0 + SFM_MIX_CHUNK;
  if (j1 > L) j1 = L;
  const long long base = ((long long)blockIdx.z * B + b) * L;
  float* o = out + base;
  const RowSplit s = row_split(base + j0, j1 - j0, vec);
  for (int q = tid; q < s.nq; q += 256) {
    const int j = j0 + s.head + 4 * q;
    f32x4 y = {0.f, 0.f, 0.f, 0.f};
    if (j < len) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      if (j + 4 <= len) {
        c = *reinterpret_cast<const f32x4_a4*>(row + j);
      } else {                           // the utterance's last quad: what follows it belongs to the next one, or to nobody
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j + k < len) c[k] = row[j + k];
      }
      if (mixed) {
        int w = mix_wrap(j, r.Ln);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (j + k < len) {
            const float z = r.noise[w];
            y[k] = c[k] + sc * z;
          }
          w = w + 1 == r.Ln ? 0 : w + 1;
        }
      } else {
        y = c;
      }
    }
    *reinterpret_cast<f32x4*>(o + j) = y;
  }
  for (int t = tid; t < s.head + s.rest; t += 256) {
    const int j = t < s.head ? j0 + t : j0 + 4 * s.nq + t;
    float y = 0.f;
    if (j < len) {
      if (mixed) {
        const float z = r.noise[mix_wrap(j, r.Ln)];
        y = row[j] + sc * z;
      } else {
        y = row[j];
      }
    }
    o[j] = y;
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------
static int ew_size(long long n) { return n <= 0 || n > 2147483647LL ? SFM_ERR_SHAPE : SFM_OK; }

extern "C" int sfm_mask_irm(const float* clean_mag, const float* noise_mag, float* out, long long n, float p, float eps,
                            void* stream) {
  if (!clean_mag || !noise_mag || !out) return SFM_ERR_ARG;
  if (!(p > 0.f) || !(eps >= 0.f)) return SFM_ERR_ARG;
  if (ew_size(n) != SFM_OK) return SFM_ERR_SHAPE;
  IrmOp op;
  op.in[0] = clean_mag, op.in[1] = noise_mag, op.out[0] = out;
  op.p = p, op.eps = eps, op.root = p == 0.5f;
  return ew_launch(op, n, stream);
}

extern "C" int sfm_mask_corr(const float* noisy, const float* clean, const float* noise, float* rho_s, float* rho_n, long long n,
                             float eps, void* stream) {
  if (!noisy || !clean || !noise || !rho_s || !rho_n || !(eps >= 0.f)) return SFM_ERR_ARG;
  if (ew_size(n) != SFM_OK) return SFM_ERR_SHAPE;
  CorrOp op;
  op.in[0] = noisy, op.in[1] = clean, op.in[2] = noise, op.out[0] = rho_s, op.out[1] = rho_n;
  op.eps = eps;
  return ew_launch(op, n, stream);
}

extern "C" int sfm_mask_pcirm(const float* clean_mag, const float* noise_mag, const float* rho_s, const float* rho_n,
                              const float* phi1, const float* phi2, float* out, long long n, float eps, void* stream) {
  if (!clean_mag || !noise_mag || !rho_s || !rho_n || !phi1 || !phi2 || !out || !(eps >= 0.f)) return SFM_ERR_ARG;
  if (ew_size(n) != SFM_OK) return SFM_ERR_SHAPE;
  PcirmOp op;
  op.in[0] = clean_mag, op.in[1] = noise_mag, op.in[2] = rho_s, op.in[3] = rho_n, op.in[4] = phi1, op.in[5] = phi2;
  op.out[0] = out;
  op.eps = eps;
  return ew_launch(op, n, stream);
}

extern "C" int sfm_mask_quantize(const float* pcirm, const double* table, float* out, long long n, int M, void* stream) {
  if (!pcirm || !table || !out) return SFM_ERR_ARG;
  if (M < 2 || M > SFM_QUANT_MAX_STEPS || ew_size(n) != SFM_OK) return SFM_ERR_SHAPE;
  QuantOp op;
  op.in[0] = pcirm, op.out[0] = out;
  op.table = table, op.M = M;
  return ew_launch(op, n, stream);
}

static int mix_check(int B, int L, int n_noise) {
  if (B <= 0 || L <= 0 || n_noise <= 0 || B > 65535) return SFM_ERR_SHAPE;
  if ((long long)B * L > 2147483647LL) return SFM_ERR_SHAPE;
  return SFM_OK;
}

static int mix_chunks(int L) { return (L + SFM_MIX_CHUNK - 1) / SFM_MIX_CHUNK; }
// ws of sfm_mix_scale: a (clean^2, noise^2) pair of partials per utterance and chunk
extern "C" long long sfm_mix_scale_ws_doubles(int B, int L) { return B > 0 && L > 0 ? 2LL * B * mix_chunks(L) : 0; }

extern "C" int sfm_mix_scale(const float* clean, const float* bank, const int* bank_off, const int* noise_ids, const float* snr_db,
                             const int* lengths, double* ws, float* scale, int B, int L, int n_noise, void* stream) {
  if (!clean || !bank || !bank_off || !noise_ids || !snr_db || !ws || !scale) return SFM_ERR_ARG;
  if (mix_check(B, L, n_noise) != SFM_OK) return SFM_ERR_SHAPE;
  const int NC = mix_chunks(L);
  hipStream_t st = (hipStream_t)stream;
  SFM_LAUNCH(mix_power_kernel, dim3((unsigned)NC, (unsigned)B), dim3(256), 0, st, clean, bank, bank_off, noise_ids, lengths, ws, L,
             n_noise, (int)al16(clean));
  SFM_LAUNCH(mix_scale_kernel, dim3(1), dim3(256), 0, st, ws, snr_db, lengths, scale, B, L, NC);
  return SFM_OK;
}

extern "C" int sfm_mix_apply(const float* clean, const float* bank, const int* bank_off, const int* noise_ids, const int* lengths,
                             const float* scale, float* noisy, float* noise_rows, int B, int L, int n_noise, void* stream) {
  if (!clean || !bank || !bank_off || !noise_ids || !scale || !noisy) return SFM_ERR_ARG;
  if (mix_check(B, L, n_noise) != SFM_OK) return SFM_ERR_SHAPE;
  const int NC = mix_chunks(L);
  const int vec = al16(clean) && al16(noisy) && al16(noise_rows);
  SFM_LAUNCH(mix_apply_kernel, dim3((unsigned)NC, (unsigned)B), dim3(256), 0, (hipStream_t)stream, clean, bank, bank_off, noise_ids,
             lengths, scale, noisy, noise_rows, L, n_noise, vec);
  return SFM_OK;
}

// ws of sfm_mix_scale_varlen: a pair of partials per utterance and chunk of the LONGEST utterance.  An int like a status: the
// count is refused (SFM_ERR_SHAPE) where it leaves 1 .. 2^31 - 1, as the entry point refuses that shape.
extern "C" int sfm_mix_scale_varlen_ws_doubles(int n_utt, int max_len) {
  if (n_utt <= 0 || max_len <= 0 || n_utt > 65535) return SFM_ERR_SHAPE;
  const long long n = 2LL * n_utt * mix_chunks(max_len);
  return n > 2147483647LL ? SFM_ERR_SHAPE : (int)n;
}

extern "C" int sfm_mix_scale_varlen(const float* packed, const int* utt_off, const float* bank, const int* bank_off,
                                    const int* noise_ids, const float* snr_db, double* ws, float* scale, int n_utt, int max_len,
                                    int total, int n_noise, void* stream) {
  if (!packed || !utt_off || !bank || !bank_off || !noise_ids || !snr_db || !ws || !scale) return SFM_ERR_ARG;
  if (total <= 0 || n_noise <= 0 || sfm_mix_scale_varlen_ws_doubles(n_utt, max_len) < 0) return SFM_ERR_SHAPE;
  const int NC = mix_chunks(max_len);
  hipStream_t st = (hipStream_t)stream;
  SFM_LAUNCH(mix_power_varlen_kernel, dim3((unsigned)NC, (unsigned)n_utt), dim3(256), 0, st, packed, utt_off, bank, bank_off,
             noise_ids, ws, total, n_noise, (int)al16(packed));
  SFM_LAUNCH(mix_scale_varlen_kernel, dim3(1), dim3(256), 0, st, ws, snr_db, utt_off, scale, n_utt, total, NC);
  return SFM_OK;
}

extern "C" int sfm_wave_batch(const float* packed, const int* utt_off, const float* bank, const int* bank_off,
                              const int* noise_ids, const float* scale, const int* index, float* out, int B, int L, int n_utt,
                              int total, int n_noise, void* stream) {
  if (!packed || !utt_off || !bank || !bank_off || !noise_ids || !scale || !index || !out) return SFM_ERR_ARG;
  if (B <= 0 || L <= 0 || n_utt <= 0 || total <= 0 || n_noise <= 0 || B > 65535) return SFM_ERR_SHAPE;
  if (2LL * B * L > 2147483647LL) return SFM_ERR_SHAPE;
  SFM_LAUNCH(wave_batch_kernel, dim3((unsigned)mix_chunks(L), (unsigned)B, 2), dim3(256), 0, (hipStream_t)stream, packed, utt_off,
             bank, bank_off, noise_ids, scale, index, out, B, L, n_utt, total, n_noise, (int)al16(out));
  return SFM_OK;
}

extern "C" int sfm_curriculum_mask(const float* cr, const float* ci, const float* nr, const float* ni, const float* scale,
                                   const double* table, float* yr, float* yi, float* mask, int B, int T, int F, int kind, float p,
                                   float eps, int M, void* stream) {
  if (!cr || !ci || !nr || !ni || !scale || !yr || !yi) return SFM_ERR_ARG;
  if (kind < SFM_MASK_NONE || kind > SFM_MASK_OPT_PCIRM || (kind != SFM_MASK_NONE && !mask) ||
      (kind == SFM_MASK_OPT_PCIRM && !table) || !(eps >= 0.f))
    return SFM_ERR_ARG;
  if (kind == SFM_MASK_IRM && !(p > 0.f)) return SFM_ERR_ARG;
  if (B <= 0 || T <= 0 || F <= 0) return SFM_ERR_SHAPE;
  if (kind == SFM_MASK_OPT_PCIRM && (M < 2 || M > SFM_QUANT_MAX_STEPS)) return SFM_ERR_SHAPE;
  const long long n = (long long)B * T * F;
  if ((long long)T * F > 2147483647LL || ew_size(n) != SFM_OK) return SFM_ERR_SHAPE;
  CurrOp op;
  op.in[0] = cr, op.in[1] = ci, op.in[2] = nr, op.in[3] = ni;
  op.out[0] = yr, op.out[1] = yi, op.out[2] = kind ? mask : nullptr;
  op.scale = scale, op.table = table;
  op.B = B, op.TF = T * F, op.kind = kind, op.M = M, op.root = p == 0.5f;
  op.p = p, op.eps = eps;
  if (op.TF < 4) {                       // a quad could cross two utterance boundaries: the scalar path
    SFM_LAUNCH((mask_ew_kernel<CurrOp>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, n, 0);
    return SFM_OK;
  }
  return ew_launch(op, n, stream);
}
