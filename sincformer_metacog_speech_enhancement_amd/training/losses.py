"""Host-side mirrors of training/losses.py: MSEMaskLoss (:22-30) and PerceptualSTOILoss (:37-143), the objectives of the
curriculum's stages 1 and 2, each one launch of curriculum_losses.hip (forward and, when the input requires it, the gradient).
The adversarial part of stage 3 (SubDiscriminator, AdversarialLoss) is not built.  How the terms are weighted and combined
is the caller's: the reference combines them nowhere."""
import numpy as np
import torch

from .. import config
from .._hostmod import HipModule

# centres of the fourteen 1/3-octave bands, 150 Hz - 3.15 kHz
BAND_CENTRES_HZ = (150, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150)
FRAME_LEN, BETA_DB = 30, 15.0
MAX_BANDS, MAX_BINS, MAX_FRAME_LEN = 32, 257, 32          # sfm_pstoi_loss


def third_octave_matrix(sample_rate, n_fft, centres=BAND_CENTRES_HZ):
    """[len(centres), n_fft // 2 + 1] float32: row i is 1 / count on the STFT bins whose frequency lies within a sixth of an
    octave of centre i (both ends included), all zero if there is none"""
    freqs = np.linspace(0, sample_rate / 2, n_fft // 2 + 1)
    w = np.zeros((len(centres), freqs.size), dtype=np.float32)
    for i, cf in enumerate(centres):
        w[i, (freqs >= cf / 2 ** (1 / 6)) & (freqs <= cf * 2 ** (1 / 6))] = 1.0
    sums = w.sum(axis=1, keepdims=True)
    sums[sums == 0] = 1.0
    return w / sums


class MSEMaskLoss(HipModule):
    def forward(self, predicted_mask, oracle_mask):
        from .. import train
        self._require_device(predicted_mask, oracle_mask)
        if predicted_mask.shape != oracle_mask.shape:
            raise ValueError("MSEMaskLoss: shapes differ: %s and %s" % (tuple(predicted_mask.shape), tuple(oracle_mask.shape)))
        return train.MseFunction.apply(predicted_mask, oracle_mask)


class PerceptualSTOILoss(HipModule):
    """-mean correlation of the mean-removed, clipped 1/3-octave envelopes over segments of `frame_len` frames.  The gradient
    goes to the enhanced side only; the clean side is a target.  `band_weights` is a buffer (it travels in state_dict) and may
    be replaced by any [NB <= 32, F <= 257] matrix; `frame_len` (2..32) and `beta` are passed to the kernel as they stand."""

    def __init__(self, sample_rate=None):
        super().__init__()
        self.num_bands = len(BAND_CENTRES_HZ)
        self.frame_len = FRAME_LEN
        self.beta = BETA_DB
        self.register_buffer("band_weights",
                             torch.from_numpy(third_octave_matrix(sample_rate or config.SAMPLE_RATE, config.FFT_SIZE)))

    def _check(self, B, T, F):
        NB, Fw = self.band_weights.shape
        FL = int(self.frame_len)
        if FL != self.frame_len or not 2 <= FL <= MAX_FRAME_LEN:
            raise NotImplementedError("PerceptualSTOILoss (HIP build): frame_len must be an integer in 2..%d" % MAX_FRAME_LEN)
        if T < FL:
            raise ValueError("PerceptualSTOILoss: %d frames are fewer than one %d-frame segment" % (T, FL))
        if F != Fw:
            raise ValueError("PerceptualSTOILoss: %d frequency bins, band_weights has %d" % (F, Fw))
        if NB > MAX_BANDS or F > MAX_BINS:
            raise ValueError("PerceptualSTOILoss (HIP build): at most %d bands and %d bins; got %d and %d"
                             % (MAX_BANDS, MAX_BINS, NB, F))
        if B < 1:
            raise ValueError("PerceptualSTOILoss: empty batch")

    def forward(self, enhanced_spec, clean_spec):
        """magnitudes [B, F, T] -> scalar"""
        from .. import train
        self._require_device(enhanced_spec, clean_spec, self.band_weights)
        if enhanced_spec.dim() != 3 or enhanced_spec.shape != clean_spec.shape:
            raise ValueError("PerceptualSTOILoss: two [B, F, T] magnitude spectrograms of one shape are needed")
        B, F, T = enhanced_spec.shape
        self._check(B, T, F)
        return train.PerceptualStoiFunction.apply(enhanced_spec, None, clean_spec, None, self.band_weights, int(self.frame_len),
                                                  float(self.beta))

    def forward_cl(self, enh_real, enh_imag, clean_real, clean_imag):
        """channels-last spectra [B, T, F] as (real, imag) pairs, as SpeechEnhancer / EnhancementPath produce them; the
        magnitudes sqrt(re^2 + im^2 + 1e-8) are taken inside the kernel -> scalar"""
        from .. import train
        self._require_device(enh_real, enh_imag, clean_real, clean_imag, self.band_weights)
        if enh_real.dim() != 3 or any(t.shape != enh_real.shape for t in (enh_imag, clean_real, clean_imag)):
            raise ValueError("PerceptualSTOILoss.forward_cl: four [B, T, F] tensors of one shape are needed")
        B, T, F = enh_real.shape
        self._check(B, T, F)
        return train.PerceptualStoiFunction.apply(enh_real, enh_imag, clean_real, clean_imag, self.band_weights,
                                                  int(self.frame_len), float(self.beta))
