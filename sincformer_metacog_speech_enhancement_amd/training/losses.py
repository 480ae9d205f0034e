"""Host-side mirrors of training/losses.py: MSEMaskLoss (:22-30) and PerceptualSTOILoss (:37-143), the objectives of the
curriculum's stages 1 and 2, each one launch of curriculum_losses.hip (forward and, when the input requires it, the gradient);
SubDiscriminator and AdversarialLoss (:150-289), the third term of stage 3: spectrally normalised Conv1d stacks at three time
scales, run as implicit GEMMs on channels-last 16-bit rows with csrc/adversarial.hip around them (train.AdversarialFunction).
How the terms are weighted and combined is the caller's: the reference combines them nowhere."""
import numpy as np
import torch
from torch import nn

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


class TaalSTOILoss(HipModule):
    """minus the mean STOI (extended: ESTOI) of Taal et al. over the utterances with at least 30 spectral frames - the measure
    evaluation.compute_stoi_taal reports, on waveforms (train.IstftFunction returns one with a graph); the sign convention of
    PerceptualSTOILoss.  An utterance below 30 frames scores a constant: it is left out of the mean and gets a zero gradient;
    with no utterance left the loss is 0.  Which utterances count is decided on the device from the kept-frame counts.  The
    gradient goes to `enhanced` only.  sample_rate 8, 10 or 16 kHz; extended=None follows config.STOI_EXTENDED at each call."""

    def __init__(self, sample_rate=None, extended=None):
        super().__init__()
        from ..evaluation.stoi_taal import check_rate
        self.sample_rate = check_rate(sample_rate or config.SAMPLE_RATE)
        self.extended = extended

    def forward(self, enhanced, clean, lengths=None):
        """fp32 device waveforms [L] or [B, L] of one shape; lengths: host sequence [B], the sample counts of zero-padded rows
        -> fp32 scalar"""
        from ..evaluation import stoi_taal as st
        self._require_device(enhanced, clean)
        ext = config.STOI_EXTENDED if self.extended is None else self.extended
        score, kept = st.scores_and_kept(enhanced, clean, self.sample_rate, bool(ext), lengths, "TaalSTOILoss")
        q = (kept > st.SEG).to(torch.float64)                  # K - 1 >= 30 spectral frames
        return (-(score * q).sum() / q.sum().clamp(min=1.0)).float()


ADV_MIN_FRAMES = 4                  # 4 -> 2 -> 1 through the two pools; at 3 the second pool has no output
ADV_CHANNELS = ((64, 128, 256, 512), (64, 128, 256), (32, 64, 128))


class SubDiscriminator(HipModule):
    """One scale: Conv1d(k 5, pad 2) per entry of `channels` (stride 2 on all but the last) + LeakyReLU(0.2) each, then
    Conv1d(C, 1, k 3, pad 1); every conv under the legacy torch.nn.utils.spectral_norm.  The convs live in `layers` at the
    reference's indices (0, 2, ..) so keys, shapes and the seeded init are its own; they are never called."""

    def __init__(self, n_freq, channels=None):
        super().__init__()
        mods, cin = [], n_freq
        channels = list(channels or ADV_CHANNELS[0])
        for i, c in enumerate(channels):
            mods += [nn.utils.spectral_norm(nn.Conv1d(cin, c, 5, stride=1 if i == len(channels) - 1 else 2, padding=2)),
                     nn.LeakyReLU(0.2, inplace=True)]
            cin = c
        mods.append(nn.utils.spectral_norm(nn.Conv1d(cin, 1, 3, padding=1)))
        self.layers = nn.Sequential(*mods)
        self.n_freq = n_freq

    def forward(self, x):
        """x [B, F, T] magnitudes -> (out [B, 1, T'], [the post-LeakyReLU features [B, C, T']]) in fp32.  A call iterates the
        spectral-norm vectors in train() like any call of the reference's; the results carry no autograd graph (the three
        objectives of AdversarialLoss are the differentiable entry points)."""
        from .. import ops, train
        self._require_device(x)
        _adv_check(self.n_freq, x, name="SubDiscriminator")
        B, F, T = x.shape
        x16, _ = ops.adv_stage(x.detach().float().contiguous(), None, ops.adv_plan(F, [1])[0][0]["Cp"], False)
        loss = torch.zeros(1, device=x.device, dtype=torch.float64)
        rec = train.adv_disc_pass(self, x16, B, T, loss, head=(0.0, 0.0))
        feats = [a.float().transpose(1, 2) for a in rec["xs"][1:]]
        return rec["out"].unsqueeze(1), feats


def _adv_check(n_freq, x, name="AdversarialLoss", cl=False):
    from .. import ops
    if n_freq > ops.ADV_MAX_WIDTH:
        raise NotImplementedError("%s (HIP build): at most %d frequency bins; got %d" % (name, ops.ADV_MAX_WIDTH, n_freq))
    if x.dim() != 3:
        raise ValueError("%s: a rank-3 spectrogram is needed; got shape %s" % (name, tuple(x.shape)))
    frames_dim, bins_dim = (1, 2) if cl else (2, 1)
    if x.shape[bins_dim] != n_freq:
        raise ValueError("%s: %d frequency bins, the discriminators take %d" % (name, x.shape[bins_dim], n_freq))
    if x.shape[frames_dim] < ADV_MIN_FRAMES or x.shape[0] < 1:
        raise ValueError("%s: at least one utterance of %d frames is needed; got shape %s" % (name, ADV_MIN_FRAMES, tuple(x.shape)))


class AdversarialLoss(HipModule):
    """Three SubDiscriminators on the input, its AvgPool1d(4, 2, 1) and the pool of that.  The three objectives take magnitudes
    [B, F, T]; the *_cl forms take channels-last spectra [B, T, F] as (real, imag) pairs, as SpeechEnhancer / EnhancementPath
    produce them (magnitude sqrt(re^2 + im^2 + 1e-8), taken in the staging kernel).  Every call of a discriminator advances its
    spectral-norm vectors in train(), so results depend on the call sequence exactly as the reference's do."""

    def __init__(self, input_dim=None):
        super().__init__()
        n_freq = input_dim or (config.FFT_SIZE // 2 + 1)
        self.discriminators = nn.ModuleList([SubDiscriminator(n_freq, list(c)) for c in ADV_CHANNELS])
        self.downsample = nn.AvgPool1d(kernel_size=4, stride=2, padding=1)     # never called: adversarial.hip's pool
        self.discriminator = self.discriminators[0]
        self.n_freq = n_freq

    def _run(self, mode, clean, clean_im, enh, enh_im, cl):
        from .. import train
        given = [t for t in (clean, clean_im, enh, enh_im) if t is not None]
        self._require_device(*given)
        for t in given[1:]:
            if t.shape != given[0].shape:
                raise ValueError("AdversarialLoss: shapes differ: %s and %s" % (tuple(given[0].shape), tuple(t.shape)))
        _adv_check(self.n_freq, enh, cl=cl)
        params = list(self.parameters())
        if any(p.dtype != torch.float32 for p in params):
            raise NotImplementedError("AdversarialLoss (HIP build): the discriminators' parameters are kept in fp32")
        return train.AdversarialFunction.apply(self, mode, clean, clean_im, enh, enh_im, *params)

    def discriminator_loss(self, clean_spec, enhanced_spec):
        return self._run("d", clean_spec, None, enhanced_spec, None, False)

    def generator_loss(self, enhanced_spec):
        return self._run("g", None, None, enhanced_spec, None, False)

    def feature_matching_loss(self, clean_spec, enhanced_spec):
        return self._run("fm", clean_spec, None, enhanced_spec, None, False)

    def discriminator_loss_cl(self, clean_real, clean_imag, enh_real, enh_imag):
        return self._run("d", clean_real, clean_imag, enh_real, enh_imag, True)

    def generator_loss_cl(self, enh_real, enh_imag):
        return self._run("g", None, None, enh_real, enh_imag, True)

    def feature_matching_loss_cl(self, clean_real, clean_imag, enh_real, enh_imag):
        return self._run("fm", clean_real, clean_imag, enh_real, enh_imag, True)
