"""Mirror of the oracle-mask recipe of training/pipeline.py:153-197: the gammatone T-F analysis of the clean, noise and noisy
waveforms (signal_processing/gammatone.py) into masks/ on the device, and of _process_single_utterance (:147-197) as a whole:
dnn_frame_pairs gives the (features, mask) pair of a batch of utterances without file I/O, cache or a host round trip, and
dnn_estimate_mask the estimator's side of enhance_signal (:846-875, its step 1): features, context and models.SpeechEnhancementDNN in
one pass.  The Dataset and the RBM are not mirrored; the Dataset's feature normalisation is an option of add_context."""
import numpy as np
import torch

from .. import config, masks
from ..signal_processing import FeatureExtractor, GammatoneFilterbank

_default_gfb = []


def gammatone_mask_target(clean, noise, noisy, mask_type, gfb=None, lengths=None):
    """-> the [B, T, C] (1-D signals: [T, C]) target 'irm', 'pcirm' or 'opt_pcirm' (the fixed steps) of fp32 device waveforms
    clean / noisy [B, L] and noise [B, Ln]; any other mask_type gives the IRM, as there.  The noise is used unscaled, trimmed or
    zero-padded to L.  The three signals are analysed in one launch over a batch of 3 B.  lengths: the sample counts of a
    zero-padded batch; frames from an utterance's T_b on are analysed as zeros.  No clipping and no nan_to_num is applied."""
    if gfb is None:
        if not _default_gfb:
            _default_gfb.append(GammatoneFilterbank())
        gfb = _default_gfb[0]
    for name, t in (("clean", clean), ("noise", noise), ("noisy", noisy)):
        if not torch.is_tensor(t) or t.dim() != clean.dim() or t.dim() not in (1, 2):
            raise ValueError("gammatone_mask_target: %s must be a tensor [L] or [B, L] like clean" % name)
    one_d = clean.dim() == 1
    c, n, y = (t.reshape(1, -1) if one_d else t for t in (clean, noise, noisy))
    B, L = c.shape
    if y.shape != c.shape or n.shape[0] != B:
        raise ValueError("gammatone_mask_target: clean %s, noise %s, noisy %s" % (tuple(c.shape), tuple(n.shape), tuple(y.shape)))
    if n.shape[1] >= L:
        n = n[:, :L]
    else:
        n = torch.nn.functional.pad(n, (0, L - n.shape[1]))
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1).repeat(3)
    mag, ph = gfb.get_tf_magnitudes(torch.cat([c, n, y], dim=0), lengths=lengths)
    clean_m, noise_m, noisy_m = mag[:B], mag[B:2 * B], mag[2 * B:]
    clean_p, noise_p, noisy_p = ph[:B], ph[B:2 * B], ph[2 * B:]
    if mask_type in ("pcirm", "opt_pcirm"):
        rho_s, rho_n = masks.compute_correlation_coefficients(noisy_m, clean_m, noise_m)
        phi1, phi2 = masks.compute_phase_differences(noisy_p, clean_p, noise_p)
        mask = masks.compute_pcirm(clean_m, noise_m, rho_s, rho_n, phi1, phi2)
        if mask_type == "opt_pcirm":
            steps, _ = masks.compute_snr_boundaries()
            mask = masks.quantize_pcirm(mask, steps)
    else:
        mask = masks.compute_irm(clean_m, noise_m)
    mask = mask.transpose(1, 2).contiguous()
    return mask[0] if one_d else mask


_default_fe = {}


def _fe_for(fe):
    if fe is None:
        if config.SAMPLE_RATE not in _default_fe:
            _default_fe[config.SAMPLE_RATE] = FeatureExtractor()
        fe = _default_fe[config.SAMPLE_RATE]
    return fe


def _frame_counts(lengths):
    """sample counts of a zero-padded batch -> frame counts T_b (numpy int64), None for None"""
    if lengths is None:
        return None
    host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    return (np.maximum(host, config.FRAME_SIZE) - config.FRAME_SIZE) // config.HOP_SIZE + 1


def dnn_frame_pairs(clean, noise, noisy, mask_type, fe=None, lengths=None, feat_mean=None, feat_std=None):
    """-> (features [B, T, 594], mask [B, T, 64]) (1-D signals: [T, 594], [T, 64]): the DNN's input rows from `noisy`
    (FeatureExtractor.extract_frame_features + add_context, normalised and clipped when feat_mean / feat_std are given) and its
    target from gammatone_mask_target, both over the same frames and with fe's one GammatoneFilterbank.  lengths: the sample counts
    of a zero-padded batch; rows from an utterance's T_b on are 0 in the features and analysed as zeros in the mask."""
    fe = _fe_for(fe)
    mask = gammatone_mask_target(clean, noise, noisy, mask_type, gfb=fe.gfb, lengths=lengths)
    raw = fe.extract_frame_features(noisy, lengths=lengths)
    return fe.add_context(raw, feat_mean, feat_std, lengths=_frame_counts(lengths)), mask


def dnn_estimate_mask(dnn, noisy, fe=None, lengths=None, feat_mean=None, feat_std=None):
    """-> the estimated mask [B, T, dnn.output_dim] (1-D signal: [T, .]) in [0, 1] of fp32 device waveforms noisy [B, L]:
    FeatureExtractor.extract_frame_features, then dnn.forward_frames (the context rows, normalised and clipped with the checkpoint's
    feat_mean / feat_std when given, are formed inside the first layer's launch), then the clip to [0, 1].  lengths: the sample counts
    of a zero-padded batch; rows from an utterance's T_b on are those of zero input rows."""
    raw = _fe_for(fe).extract_frame_features(noisy, lengths=lengths)
    return dnn.forward_frames(raw, feat_mean, feat_std, lengths=_frame_counts(lengths)).clamp_(0.0, 1.0)
