// On-device quality metrics of the step right after the path (main.py:141-151 evaluates every utterance with
// evaluation/ssnr.py:26 and the fallback STOI of evaluation/stoi.py:53 in per-utterance numpy loops): batched here.
//   ssnr_frames : per 160-sample frame (hop 80) 10 log10(sum c^2 / sum (c - e)^2), clipped, silence skipped;
//                 per-utterance sum and count in fp64 (evaluation/ssnr.py:53-92)
//   stoi_frames : per analysis frame the normalised spectral correlation of evaluation/stoi.py:76-94 from the two
//                 magnitude spectra (the DFTs run on framed_gemm_f32 with the symmetric-Hann DFT operand)
//   lsd_frames  : per analysis frame the log-spectral distortion of the reference's PESQ fallback
//                 (evaluation/pesq_eval.py:66-78) from the two spectra of a rectangular-window DFT
// Each has a packed (_varlen) form for utterances of different lengths back to back: samples [samp_off[u], samp_off[u + 1]),
// frames / spectrum rows [frame_off[u], frame_off[u + 1]) - the metric's OWN framing, an utterance may own no frame at all.
#include "sfm_common.h"

// acc[b] = { sum of kept frame SNRs, number of kept frames }
__global__ __launch_bounds__(256) void ssnr_frames_kernel(const float* __restrict__ clean, const float* __restrict__ enh,
                                                          double* __restrict__ acc, int L, int nframes, int frame, int hop,
                                                          float upper, float lower) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const float* c = clean + (long long)b * L;
  const float* e = enh + (long long)b * L;
  double ssum = 0.0, scnt = 0.0;
  for (int n = blockIdx.x * 4 + wave; n < nframes; n += gridDim.x * 4) {
    const int start = n * hop;
    double sp = 0.0, ep = 0.0;
    for (int i = lane; i < frame; i += 64) {
      const double cv = c[start + i], d = cv - (double)e[start + i];
      sp += cv * cv;
      ep += d * d;
    }
    sp = wave_sum_d(sp);
    ep = wave_sum_d(ep);
    if (sp < 1e-10) continue;                                  // silence frame: skipped (evaluation/ssnr.py:72)
    double snr = (ep < 1e-10) ? (double)upper : 10.0 * log10(sp / ep);
    snr = fmin(fmax(snr, (double)lower), (double)upper);
    ssum += snr;
    scnt += 1.0;
  }
  if (lane == 0 && scnt > 0.0) {
    atomicAdd(&acc[2 * b + 0], ssum);
    atomicAdd(&acc[2 * b + 1], scnt);
  }
}

// Packed form: one wave per PACKED frame, so a pass costs sum n_u frames.  A wave owns a run of consecutive packed frames
// (the launch's waves split [0, sum_n) evenly), looks the utterance of its first frame up once and then walks the offsets;
// when the utterance changes it flushes its fp64 partial (sfm_seg_find and the walk both step over utterances without frames).
// A frame that would reach past its utterance's last sample (tables that disagree with frame / hop) is not read.
__global__ __launch_bounds__(256) void ssnr_frames_varlen_kernel(const float* __restrict__ clean, const float* __restrict__ enh,
                                                                 double* __restrict__ acc, const int* __restrict__ samp_off,
                                                                 const int* __restrict__ frame_off, int B, int sum_n, int frame,
                                                                 int hop, float upper, float lower) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long nw = (long long)gridDim.x * 4;
  const long long per = (sum_n + nw - 1) / nw;
  const long long first = (blockIdx.x * 4LL + wave) * per;
  if (first >= sum_n) return;
  const int end = (int)(first + per < sum_n ? first + per : sum_n);
  int n = (int)first;
  int u = sfm_seg_find(frame_off, B, n);
  int fo = frame_off[u], fe = frame_off[u + 1];
  double ssum = 0.0, scnt = 0.0;
  for (; n < end; ++n) {
    if (n >= fe) {                                             // the next utterance that owns a frame
      if (lane == 0 && scnt > 0.0) {
        atomicAdd(&acc[2 * u + 0], ssum);
        atomicAdd(&acc[2 * u + 1], scnt);
      }
      ssum = 0.0;
      scnt = 0.0;
      while (u + 1 < B && n >= fe) fe = frame_off[++u + 1];
      if (n >= fe) return;                                     // sum_n beyond frame_off[B]: nothing is read
      fo = frame_off[u];
    }
    const long long start = (long long)samp_off[u] + (long long)(n - fo) * hop;
    if (start + frame > samp_off[u + 1]) continue;
    double sp = 0.0, ep = 0.0;
    for (int i = lane; i < frame; i += 64) {
      const double cv = clean[start + i], d = cv - (double)enh[start + i];
      sp += cv * cv;
      ep += d * d;
    }
    sp = wave_sum_d(sp);
    ep = wave_sum_d(ep);
    if (sp < 1e-10) continue;
    double snr = (ep < 1e-10) ? (double)upper : 10.0 * log10(sp / ep);
    snr = fmin(fmax(snr, (double)lower), (double)upper);
    ssum += snr;
    scnt += 1.0;
  }
  if (lane == 0 && scnt > 0.0) {
    atomicAdd(&acc[2 * u + 0], ssum);
    atomicAdd(&acc[2 * u + 1], scnt);
  }
}

// One template for the two per-frame spectral measures, dense and packed.  Spectra (real, imag) of the RAW signals, fp32 in,
// fp64 arithmetic and sums.
//   MODE_STOI: sc[b], se[b] = the rms normalisation factors 1/(rms + 1e-10) of evaluation/stoi.py:65-66 (spectra are linear in
//              the signal); acc[b] += clip(corr, -1, 1)
//   MODE_LSD : acc[b] += sqrt(mean_f (log(|C_f| + 1e-10) - log(|E_f| + 1e-10))^2)   (sc / se are not read)
// dense : spectra [B, nframes, F], grid (blocks, B), the waves stride over the utterance's frames
// VARLEN: spectra rows [sum_n, F] (nframes = sum_n), utterance u owns rows [frame_off[u], frame_off[u + 1]); grid (blocks),
//         a wave owns a run of consecutive rows and flushes when the utterance changes, as ssnr_frames_varlen_kernel
enum { MODE_STOI = 0, MODE_LSD = 1 };

template <int MODE>
__device__ __forceinline__ double spec_frame_value(const float* __restrict__ cr, const float* __restrict__ ci,
                                                   const float* __restrict__ er, const float* __restrict__ ei, long long off, int F,
                                                   int lane, double kc, double ke) {
  if (MODE == MODE_STOI) {
    double A = 0.0, Bq = 0.0, C = 0.0;
    for (int f = lane; f < F; f += 64) {
      const double a0 = cr[off + f], a1 = ci[off + f], b0 = er[off + f], b1 = ei[off + f];
      const double cm = sqrt(a0 * a0 + a1 * a1) * kc, em = sqrt(b0 * b0 + b1 * b1) * ke;
      A += cm * cm;
      Bq += em * em;
      C += cm * em;
    }
    A = wave_sum_d(A);
    Bq = wave_sum_d(Bq);
    C = wave_sum_d(C);
    const double clean_energy = sqrt(A + 1e-10);
    const double k = clean_energy / (sqrt(Bq) + 1e-10);        // enh_norm = enh_spec * k
    const double corr = (k * C) / (sqrt(A * (k * k * Bq)) + 1e-10);
    return fmin(fmax(corr, -1.0), 1.0);
  } else {
    double D = 0.0;
    for (int f = lane; f < F; f += 64) {
      const double a0 = cr[off + f], a1 = ci[off + f], b0 = er[off + f], b1 = ei[off + f];
      const double d = log(sqrt(a0 * a0 + a1 * a1) + 1e-10) - log(sqrt(b0 * b0 + b1 * b1) + 1e-10);
      D += d * d;
    }
    return sqrt(wave_sum_d(D) / (double)F);
  }
}

template <int MODE, bool VARLEN>
__global__ __launch_bounds__(256) void spec_frames_kernel(const float* __restrict__ cr, const float* __restrict__ ci,
                                                          const float* __restrict__ er, const float* __restrict__ ei,
                                                          const double* __restrict__ sc, const double* __restrict__ se,
                                                          double* __restrict__ acc, const int* __restrict__ frame_off, int B,
                                                          int nframes, int F) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (!VARLEN) {
    const int b = blockIdx.y;
    const double kc = MODE == MODE_STOI ? sc[b] : 1.0, ke = MODE == MODE_STOI ? se[b] : 1.0;
    double total = 0.0;
    for (int n = blockIdx.x * 4 + wave; n < nframes; n += gridDim.x * 4)
      total += spec_frame_value<MODE>(cr, ci, er, ei, ((long long)b * nframes + n) * F, F, lane, kc, ke);
    if (lane == 0) atomicAdd(&acc[b], total);
  } else {
    const long long nw = (long long)gridDim.x * 4;
    const long long per = (nframes + nw - 1) / nw;
    const long long first = (blockIdx.x * 4LL + wave) * per;
    if (first >= nframes) return;
    const int end = (int)(first + per < nframes ? first + per : nframes);
    int n = (int)first;
    int u = sfm_seg_find(frame_off, B, n);
    int fe = frame_off[u + 1];
    double kc = MODE == MODE_STOI ? sc[u] : 1.0, ke = MODE == MODE_STOI ? se[u] : 1.0;
    double total = 0.0;
    for (; n < end; ++n) {
      if (n >= fe) {
        if (lane == 0) atomicAdd(&acc[u], total);
        total = 0.0;
        while (u + 1 < B && n >= fe) fe = frame_off[++u + 1];
        if (n >= fe) return;                                   // rows beyond frame_off[B] belong to nobody
        if (MODE == MODE_STOI) { kc = sc[u]; ke = se[u]; }
      }
      total += spec_frame_value<MODE>(cr, ci, er, ei, (long long)n * F, F, lane, kc, ke);
    }
    if (lane == 0) atomicAdd(&acc[u], total);
  }
}

static int frame_blocks(int nframes, int cap) {
  int nb = (nframes + 3) / 4;
  return nb > cap ? cap : nb;
}

extern "C" int sfm_ssnr_frames(const float* clean, const float* enh, double* acc, int B, int L, int frame, int hop,
                               float upper, float lower, void* stream) {
  if (!clean || !enh || !acc) return SFM_ERR_ARG;
  if (B <= 0 || L <= 0 || frame <= 0 || hop <= 0) return SFM_ERR_SHAPE;
  const int nframes = (L - frame) / hop + 1;
  if (L < frame || nframes < 1) return SFM_OK;                 // fewer samples than one frame: acc stays {0, 0}
  int nb = (nframes + 3) / 4;
  if (nb > 256) nb = 256;
  SFM_LAUNCH(ssnr_frames_kernel, dim3(nb, B), dim3(256), 0, (hipStream_t)stream, clean, enh, acc, L, nframes, frame, hop, upper,
             lower);
  return SFM_OK;
}

// Packed forms: sum_frames = frame_off[B] (0: no utterance owns a frame, nothing is launched, acc stays zero)
extern "C" int sfm_ssnr_frames_varlen(const float* clean, const float* enh, double* acc, const int* samp_off,
                                      const int* frame_off, int B, int sum_frames, int frame, int hop, float upper, float lower,
                                      void* stream) {
  if (!clean || !enh || !acc || !samp_off || !frame_off) return SFM_ERR_ARG;
  if (B <= 0 || sum_frames < 0 || frame <= 0 || hop <= 0) return SFM_ERR_SHAPE;
  if (sum_frames == 0) return SFM_OK;
  SFM_LAUNCH(ssnr_frames_varlen_kernel, dim3(frame_blocks(sum_frames, 2048)), dim3(256), 0, (hipStream_t)stream, clean, enh, acc,
             samp_off, frame_off, B, sum_frames, frame, hop, upper, lower);
  return SFM_OK;
}

extern "C" int sfm_stoi_frames(const float* cr, const float* ci, const float* er, const float* ei, const double* sc,
                               const double* se, double* acc, int B, int nframes, int F, void* stream) {
  if (!cr || !ci || !er || !ei || !sc || !se || !acc) return SFM_ERR_ARG;
  if (B <= 0 || nframes <= 0 || F <= 0) return SFM_ERR_SHAPE;
  SFM_LAUNCH((spec_frames_kernel<MODE_STOI, false>), dim3(frame_blocks(nframes, 256), B), dim3(256), 0, (hipStream_t)stream, cr, ci,
             er, ei, sc, se, acc, (const int*)nullptr, B, nframes, F);
  return SFM_OK;
}

extern "C" int sfm_stoi_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, const double* sc,
                                      const double* se, double* acc, const int* frame_off, int B, int sum_frames, int F,
                                      void* stream) {
  if (!cr || !ci || !er || !ei || !sc || !se || !acc || !frame_off) return SFM_ERR_ARG;
  if (B <= 0 || sum_frames < 0 || F <= 0) return SFM_ERR_SHAPE;
  if (sum_frames == 0) return SFM_OK;
  SFM_LAUNCH((spec_frames_kernel<MODE_STOI, true>), dim3(frame_blocks(sum_frames, 2048)), dim3(256), 0, (hipStream_t)stream, cr, ci,
             er, ei, sc, se, acc, frame_off, B, sum_frames, F);
  return SFM_OK;
}

extern "C" int sfm_lsd_frames(const float* cr, const float* ci, const float* er, const float* ei, double* acc, int B, int nframes,
                              int F, void* stream) {
  if (!cr || !ci || !er || !ei || !acc) return SFM_ERR_ARG;
  if (B <= 0 || nframes <= 0 || F <= 0) return SFM_ERR_SHAPE;
  SFM_LAUNCH((spec_frames_kernel<MODE_LSD, false>), dim3(frame_blocks(nframes, 256), B), dim3(256), 0, (hipStream_t)stream, cr, ci,
             er, ei, (const double*)nullptr, (const double*)nullptr, acc, (const int*)nullptr, B, nframes, F);
  return SFM_OK;
}

extern "C" int sfm_lsd_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, double* acc,
                                     const int* frame_off, int B, int sum_frames, int F, void* stream) {
  if (!cr || !ci || !er || !ei || !acc || !frame_off) return SFM_ERR_ARG;
  if (B <= 0 || sum_frames < 0 || F <= 0) return SFM_ERR_SHAPE;
  if (sum_frames == 0) return SFM_OK;
  SFM_LAUNCH((spec_frames_kernel<MODE_LSD, true>), dim3(frame_blocks(sum_frames, 2048)), dim3(256), 0, (hipStream_t)stream, cr, ci,
             er, ei, (const double*)nullptr, (const double*)nullptr, acc, frame_off, B, sum_frames, F);
  return SFM_OK;
}
