"""evaluation/ncm.py: the normalised covariance metric, batched on the device.

Per gammatone channel the reference takes the Hilbert envelopes |scipy.signal.hilbert(.)| of the filtered clean and enhanced
signal and their normalised covariance; the score is the importance-weighted sum of the non-negative ones.  hilbert(x).imag is
the circular convolution of x with a fixed kernel h (ops.hilbert_kernel_table; one table per distinct length, cached on the host), so no FFT is needed: the filtered planes of
GammatoneFilterbank.filter go through the fp32 matrix cores once more (csrc/intelligibility.hip), the envelopes are formed in
the kernel's epilogue and only five fp64 sums per (utterance, channel, output tile) reach memory."""
import numpy as np
import torch

from .. import config, ops
from ..signal_processing.gammatone import GammatoneFilterbank
from ._common import to_device_batch

MIN_LEN = 64                                                  # ncm.py:83: shorter signals score 0.0
GROUP_BYTES = 256 << 20                                       # filtered planes held at a time by the packed form
_banks = {}
_wts = {}


def default_bank(fs=None):
    """the GammatoneFilterbank(sample_rate=fs) the reference builds per call (ncm.py:87-88), built once per fs"""
    fs = fs or config.SAMPLE_RATE
    if fs not in _banks:
        _banks[fs] = GammatoneFilterbank(sample_rate=fs)
    return _banks[fs]


def channel_weights(center_freqs):
    """float64 [C]: the importance weights of ncm.py:106-119"""
    cf = np.asarray(center_freqs, dtype=np.float64)
    w = np.select([cf < 300, cf < 1000, cf < 3400], [0.3, 0.8, 1.0], 0.5)
    return w / np.sum(w)


def _weights(gfb, dev):
    key = (id(gfb), str(dev))
    if key not in _wts:
        _wts[key] = (gfb, torch.from_numpy(channel_weights(gfb.center_freqs)).to(dev))
    return _wts[key][1]


def plan_groups(lengths, num_channels, budget=None):
    """host: [(start, stop)] over the utterances in their order, cut greedily so that a group's filtered planes, padded to its
    longest utterance (2 x C x L x 4 bytes each), stay under `budget` bytes; an utterance above the budget is a group of its own"""
    budget = GROUP_BYTES if budget is None else int(budget)
    groups, start, longest = [], 0, 0
    for i, L in enumerate(int(x) for x in lengths):
        if i > start and (i - start + 1) * max(longest, L) * 8 * num_channels > budget:
            groups.append((start, i))
            start, longest = i, 0
        longest = max(longest, L)
    if len(lengths) > start:
        groups.append((start, len(lengths)))
    return groups


def ncm_padded(clean, enhanced, lengths, gfb, want_ncc=False):
    """clean, enhanced [B, L] fp32 device tensors, utterance b = its first lengths[b] samples (host integers) -> score [B] fp64
    (and ncc [B, C] fp64: the clipped normalised covariance per channel).  An utterance gets the bits it gets alone."""
    dev, (B, L) = clean.device, clean.shape
    C = gfb.num_channels
    if C > ops.GT_COLS:
        raise ValueError("compute_ncm: %d channels; the kernels take <= %d" % (C, ops.GT_COLS))
    host = np.asarray(lengths, dtype=np.int64).reshape(-1)
    tiles, tile_off, work = ops.hilbert_tiles(host, MIN_LEN)
    distinct = sorted(set(int(x) for x in host if x >= MIN_LEN))
    if not distinct:
        z = torch.zeros(B, device=dev, dtype=torch.float64)
        return (z, torch.zeros(B, C, device=dev, dtype=torch.float64)) if want_ncc else z
    where = dict(zip(distinct, np.concatenate([[0], np.cumsum([2 * x for x in distinct])])))
    tables = ops.hilbert_table(distinct, dev)
    tab_off = np.asarray([where.get(int(x), 0) for x in host], dtype=np.int32)
    flat = torch.from_numpy(np.concatenate([host.astype(np.int32), tab_off, tile_off, tiles.reshape(-1)])).to(dev)
    len_d, tab_off_d, tile_off_d = flat[:B], flat[B:2 * B], flat[2 * B:3 * B + 1]
    tiles_d = flat[3 * B + 1:].view(-1, 2)
    X = gfb.filter(torch.cat([clean, enhanced]), lengths=np.concatenate([np.maximum(host, 1)] * 2))      # [2 B, C, L]
    partial = ops.hilbert_env_moments(X.view(2, B, C, L), tables, tab_off_d, len_d, tiles_d, C, work)
    score, ncc = ops.ncm_finish(partial, tile_off_d, len_d, _weights(gfb, dev), B, C)
    return (score, ncc) if want_ncc else score


def compute_ncm(clean_signal, enhanced_signal, fs=None, gfb=None, want_ncc=False):
    """1-D inputs -> float (the reference's signature); [B, L] inputs -> tensor [B] fp64 (stays on the device).  gfb: a
    signal_processing.GammatoneFilterbank (at most 64 channels); default the bank of fs.  want_ncc=True returns (score, ncc)."""
    (c, e), one_d = to_device_batch(clean_signal, enhanced_signal)
    B, L = c.shape
    gfb = gfb or default_bank(fs)
    if L < MIN_LEN:
        out = (torch.zeros(B, device=c.device, dtype=torch.float64),
               torch.zeros(B, gfb.num_channels, device=c.device, dtype=torch.float64))
    else:
        out = ncm_padded(c, e, np.full(B, L), gfb, True)
    score, ncc = (float(out[0][0]), out[1][0]) if one_d else out
    return (score, ncc) if want_ncc else score


def hilbert_envelope(x):
    """|scipy.signal.hilbert(x)| along the last axis of an fp32 device tensor [L] or [R, L], on the matrix cores"""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("hilbert_envelope: the sincformer HIP path only runs on an MI355X device tensor (no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() not in (1, 2) or x.numel() == 0:
        raise ValueError("hilbert_envelope: an fp32 tensor [L] or [R, L] is needed; got %s %s" % (x.dtype, tuple(x.shape)))
    env = ops.hilbert_env(x.detach().reshape(-1, x.shape[-1]).contiguous())
    return env.reshape(x.shape)
