"""Mirror of the oracle-mask recipe of training/pipeline.py:153-197: the gammatone T-F analysis of the clean, noise and noisy
waveforms (signal_processing/gammatone.py) into masks/ on the device, and of _process_single_utterance (:147-197) as a whole:
dnn_frame_pairs gives the (features, mask) pair of a batch of utterances without file I/O, cache or a host round trip, and
dnn_estimate_mask the estimator's side of enhance_signal (:846-875, its step 1): features, context and models.SpeechEnhancementDNN in
one pass; resynthesize its steps 2-4 (:877-934): the STFT of the noisy signal, the mask interpolated onto the STFT bins, the masked
irfft and the overlap-add in one launch; dnn_enhance_signal the two together; rbm_pretrain is _rbm_pretrain (:712-759), the layer-wise
RBM pre-training of the DNN on models.rbm.  The Dataset and the training loop are in training/dnn_training.py (FrameSet,
TrainingPipeline); the Dataset's feature normalisation is also an option of add_context."""
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
    of a zero-padded batch; rows from an utterance's T_b on are those of zero input rows.  Under autograd (dnn in train() or with
    enable_eval_autograd()) the mask carries the history of train.DnnFunction and the clip is out of place - the node keeps its
    output for its backward - and passes the gradient on [0, 1] inclusive, as torch.clamp does."""
    raw = _fe_for(fe).extract_frame_features(noisy, lengths=lengths)
    mask = dnn.forward_frames(raw, feat_mean, feat_std, lengths=_frame_counts(lengths))
    return mask.clamp(0.0, 1.0) if mask.requires_grad else mask.clamp_(0.0, 1.0)


_default_cf = []


def resynthesize(noisy, mask, lengths=None, fs=None, center_freqs=None, *, frame=None, hop=None, n_fft=None):
    """-> the enhanced waveforms [B, L] (1-D signal: [L]) fp32, steps 2-4 of enhance_signal (:877-934) in one launch
    (ops.mask_resynth): the Hann STFT of fp32 device waveforms noisy [B, L], the mask [B, T_mask, C] ([T_mask, C]) interpolated from
    its channels' centre frequencies onto the STFT bins as np.interp does (a bin below the first channel takes the first, one above
    the last takes the last), the masked irfft, the overlap-add and the division by the window sum.  Frames from min(T_b, T_mask)
    on contribute nothing; samples no such frame covers are 0, so an utterance shorter than one frame gives zeros (the reference
    raises below one hop).  The mask is used as given: the clip to [0, 1] is dnn_estimate_mask's.  lengths: the sample counts of a
    zero-padded batch.  fs: config.SAMPLE_RATE; center_freqs: erb_space(FREQ_LOW, FREQ_HIGH, NUM_CHANNELS), any ascending
    frequencies, one per mask channel; frame, hop, n_fft: config's framing.
    Autograd: when it is enabled and the mask requires a gradient, the result carries train.ResynthFunction, whose backward is one
    launch of the adjoint in the mask (ops.mask_resynth_bwd; the waveform is linear in the mask); the forward's bits are the same.
    In every other case the result has no history.  The gradient to `noisy` does not exist here: a noisy signal that requires one
    raises NotImplementedError under autograd, and the node has no second derivative."""
    fs = config.SAMPLE_RATE if fs is None else fs
    frame = config.FRAME_SIZE if frame is None else int(frame)
    hop = config.HOP_SIZE if hop is None else int(hop)
    n_fft = config.FFT_SIZE if n_fft is None else int(n_fft)
    if center_freqs is None:
        if not _default_cf:
            from ..signal_processing.gammatone import erb_space
            _default_cf.append(np.asarray(erb_space(config.FREQ_LOW, config.FREQ_HIGH, config.NUM_CHANNELS), dtype=np.float64))
        center_freqs = _default_cf[0]
    cf = np.asarray(center_freqs, dtype=np.float64).reshape(-1)
    for name, t, dims in (("noisy", noisy, (1, 2)), ("mask", mask, (2, 3))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in dims:
            raise ValueError("resynthesize: %s must be an fp32 tensor of %d or %d dimensions" % ((name,) + dims))
    if (noisy.dim() == 1) != (mask.dim() == 2):
        raise ValueError("resynthesize: noisy %s and mask %s: both batched or both single" % (tuple(noisy.shape), tuple(mask.shape)))
    if torch.is_grad_enabled() and noisy.requires_grad:
        raise NotImplementedError("resynthesize: the gradient with respect to the noisy signal is not implemented (only the mask's "
                                  "is: ops.mask_resynth_bwd); detach `noisy`")
    one_d = noisy.dim() == 1
    y, m = (noisy.reshape(1, -1), mask.unsqueeze(0)) if one_d else (noisy, mask)
    B, L = y.shape
    if m.shape[0] != B:
        raise ValueError("resynthesize: %d waveforms, %d masks" % (B, m.shape[0]))
    if m.shape[2] != cf.size:
        raise ValueError("resynthesize: the mask has %d channels, there are %d centre frequencies" % (m.shape[2], cf.size))
    if cf.size < 2 or not np.all(np.diff(cf) > 0):
        raise ValueError("resynthesize: the centre frequencies must be strictly ascending")
    from .. import ops
    if not ops.resynth_supported(frame, hop, n_fft, cf.size):
        raise ValueError("resynthesize: frame %d, hop %d, n_fft %d, %d channels: hop * 2 == frame <= n_fft <= %d, n_fft even and 2 .. %d "
                         "channels are supported" % (frame, hop, n_fft, cf.size, ops.RESYNTH_MAX_NFFT, ops.RESYNTH_MAX_CHANNELS))
    if B == 0 or L == 0 or m.shape[1] == 0:
        raise ValueError("resynthesize: empty noisy %s or mask %s" % (tuple(noisy.shape), tuple(mask.shape)))
    if not y.is_cuda or m.device != y.device:
        raise ValueError("resynthesize: noisy (%s) and mask (%s) must be on one device; there is no host path" % (y.device, m.device))
    T_mask = m.shape[1]
    dev_lengths = None
    host = np.full(B, L, dtype=np.int64)
    if lengths is not None:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
        if host.size != B:
            raise ValueError("resynthesize: %d lengths for %d waveforms" % (host.size, B))
        host = np.clip(host, 0, L)
        dev_lengths = torch.from_numpy(host.astype(np.int32)).to(y.device)
    frames = int(np.minimum(np.where(host >= frame, (host - frame) // hop + 1, 0), T_mask).sum())
    if torch.is_grad_enabled() and m.requires_grad:
        from .. import train
        out = train.ResynthFunction.apply(y.detach().contiguous(), m.contiguous(), dev_lengths, frames,
                                          dict(frame=frame, hop=hop, n_fft=n_fft, fs=fs, cf=cf))
    else:
        out = ops.mask_resynth(y.detach().contiguous(), m.detach().contiguous(), dev_lengths, frame=frame, hop=hop, n_fft=n_fft, fs=fs,
                               cf=cf, frames=frames)
    return out[0] if one_d else out


def dnn_enhance_signal(dnn, noisy, fe=None, lengths=None, feat_mean=None, feat_std=None):
    """-> the enhanced waveforms [B, L] (1-D signal: [L]): the whole of enhance_signal (:819-934) for a batch,
    resynthesize(noisy, dnn_estimate_mask(dnn, noisy, ...), lengths) with config's framing and centre frequencies.  With dnn in
    train() or with enable_eval_autograd() the result is differentiable with respect to the DNN's parameters (train.DnnFunction,
    the clip, train.ResynthFunction), so a waveform objective trains the mask estimator, e.g.
    TaalSTOILoss(extended=True)(dnn_enhance_signal(dnn, noisy, lengths=l), clean, l).backward(); in eval() without it nothing is
    recorded."""
    return resynthesize(noisy, dnn_estimate_mask(dnn, noisy, fe=fe, lengths=lengths, feat_mean=feat_mean, feat_std=feat_std), lengths)


def rbm_weights_degenerate(rbm_weights):
    """the reference's check (:750-756): the index of the first layer whose W has np.std below 1e-6 or NaN, None when every layer is
    fine.  Tensors (one readback for the whole stack) or numpy arrays."""
    if all(torch.is_tensor(w) for w, _, _ in rbm_weights):
        stds = torch.stack([w.detach().double().std(unbiased=False) for w, _, _ in rbm_weights]).cpu().numpy()
    else:
        stds = np.array([np.std(np.asarray(w.detach().cpu() if torch.is_tensor(w) else w, dtype=np.float64)) for w, _, _ in rbm_weights])
    for i, w_std in enumerate(stds):
        if w_std < 1e-6 or np.isnan(w_std):
            return i
    return None


def rbm_pretrain(dnn, features, max_samples=50000, seed=None, verbose=True):
    """_rbm_pretrain (:712-759) on the device: at most max_samples rows of the normalised features [N, dnn.input_dim] (fp32 device
    tensor; what dnn_frame_pairs returns with statistics, flattened over utterances) are squashed with RBM.sigmoid, a stack of RBMs
    of sizes [input_dim] + [hidden_dim] * num_hidden_layers is trained on them (models.pretrain_dnn_with_rbm, counter mode with
    `seed`), and - unless a layer's weights are degenerate (std < 1e-6 or NaN: nothing is loaded, False) - loaded into the DNN's
    hidden Linears (True).  The output layer is never set."""
    from ..models.rbm import RBM, pretrain_dnn_with_rbm
    if not torch.is_tensor(features) or features.dtype != torch.float32 or features.dim() < 2 or features.shape[-1] != dnn.input_dim:
        raise ValueError("rbm_pretrain: fp32 features [..., %d] are needed" % dnn.input_dim)
    if not features.is_cuda:
        raise RuntimeError("rbm_pretrain: the RBM only runs on an MI355X device tensor; got a CPU tensor (there is no CPU fallback)")
    rbm_data_01 = RBM.sigmoid(features.detach().reshape(-1, dnn.input_dim)[:max_samples]).contiguous()
    layer_sizes = [dnn.input_dim] + [dnn.hidden_dim] * dnn.num_hidden_layers
    if verbose:
        print(f"  RBM data: {rbm_data_01.shape[0]:,} samples, dim={rbm_data_01.shape[1]}")
    rbm_weights = pretrain_dnn_with_rbm(rbm_data_01, layer_sizes, verbose=verbose, seed=seed)
    bad = rbm_weights_degenerate(rbm_weights)
    if bad is not None:
        if verbose:
            print(f"  RBM layer {bad+1} weights degenerate. Skipping load.")
        return False
    dnn.load_rbm_weights(rbm_weights)
    if verbose:
        print("  RBM weights loaded into DNN")
    return True
