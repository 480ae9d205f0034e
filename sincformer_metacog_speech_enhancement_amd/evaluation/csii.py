"""evaluation/csii.py: the coherence speech intelligibility index, batched on the device.

The reference sorts the frames of the clean signal into `num_levels` amplitude regions (_split_by_amplitude) and then, for
every region, calls _magnitude_squared_coherence on the WHOLE signal (csii.py:190-193); every non-empty region holds at least one
frame of samples, so with frame = int(0.016 fs), hop = frame // 2 the value is

    0.0                                 when min_len < frame
    clip(sum_f w_f msc_f, 0, 1)         otherwise: one coherence estimate over all (min_len - frame) // hop + 1 frames

whatever num_levels >= 1.  Nothing is sorted here.  The one difference: num_levels = 0 is nan in the
reference (the mean of no level) and a ValueError here.

The analysis DFT is rfft(frame * hamming(frame), n=256): a frame shorter than 256 is zero padded (8 kHz: 128 samples), a longer
one cropped to its first 256 windowed samples (above 16 kHz) while the frame count still uses the full frame."""
import numpy as np
import torch

from .. import config, functional as Fn, ops
from ._common import to_device_batch

N_FFT = 256
_mat = {}
_wts = {}


def csii_framing(fs=None):
    """(frame, hop): 16 ms frames of fs, half overlap (csii.py:166-167)"""
    frame = int(0.016 * (fs or config.SAMPLE_RATE))
    return frame, frame // 2


def sii_weights(fs=None):
    """float64 [129]: _speech_importance_function(129, fs, 256) of the reference (csii.py:71-97)"""
    fs = fs or config.SAMPLE_RATE
    f = np.arange(N_FFT // 2 + 1) * fs / N_FFT
    w = np.select([f < 200, f < 500, f < 1000, f < 2000, f < 4000], [0.0, 0.5, 0.8, 1.0, 0.9], 0.4)
    return w / (np.sum(w) + 1e-10)


def _weights(fs, dev):
    key = (fs, str(dev))
    if key not in _wts:
        _wts[key] = torch.from_numpy(sii_weights(fs)).to(dev)
    return _wts[key]


def csii_operand_host(fs=None):
    """float64 [K, 258], K = min(frame, 256): rows n of [w cos | -w sin](2 pi ((n f) mod 256) / 256), w = hamming(frame)[:K]"""
    frame, _ = csii_framing(fs)
    K = min(frame, N_FFT)
    w = np.hamming(frame)[:K] if frame > 1 else np.ones(K)
    n = np.arange(K, dtype=np.int64)[:, None]
    f = np.arange(N_FFT // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * f) % N_FFT).astype(np.float64) / N_FFT
    return np.concatenate([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)], axis=1)


def _operand(fs, dev):
    key = (csii_framing(fs)[0], str(dev))
    if key not in _mat:
        _mat[key] = ops.pack_f32_matrix(torch.from_numpy(csii_operand_host(fs).astype(np.float32)).to(dev))
    return _mat[key]


def _check_levels(num_levels):
    if int(num_levels) < 1:
        raise ValueError("compute_csii: num_levels %r; at least 1 is needed (the reference's mean over no level is nan)" % (num_levels,))


def csii_packed(clean, enhanced, seg, fs=None, want_msc=False):
    """clean, enhanced: [sum_L] fp32 device tensors holding the utterances of `seg` back to back -> score [B] fp64 (and the msc
    plane [B, 129] fp64).  Nothing in here waits for the device."""
    fs = fs or config.SAMPLE_RATE
    dev, B = clean.device, seg.B
    frame, hop = csii_framing(fs)
    if frame < 2:
        raise ValueError("compute_csii: fs %r gives a frame of %d samples" % (fs, frame))
    tab = seg.metric_tables(dev, ((frame, hop),))[(frame, hop)]
    if tab["sum"] == 0:
        z = torch.zeros(B, device=dev, dtype=torch.float64)
        return (z, torch.zeros(B, ops.CSII_BINS, device=dev, dtype=torch.float64)) if want_msc else z
    W = _operand(fs, dev)
    samp_off = seg.tables(dev)["samp_off"]
    F, K = ops.CSII_BINS, min(frame, N_FFT)
    planes = torch.empty(4, tab["sum"], F, device=dev, dtype=torch.float32)
    for i, sig in enumerate((clean, enhanced)):
        ops.framed_gemm_varlen(sig, W, planes[2 * i], samp_off, tab["frame_off"], B=B, sum_T=tab["sum"], hop=hop, padl=0, K=K,
                               N=2 * F, ldm=F, mode=0, out2=planes[2 * i + 1], nsplit=F)
    return ops.csii_frames_varlen(planes[0], planes[1], planes[2], planes[3], tab["frame_off"], _weights(fs, dev), B, want_msc)


def compute_csii(clean_signal, enhanced_signal, fs=None, num_levels=3, want_msc=False):
    """1-D inputs -> float (the reference's signature); [B, L] inputs -> tensor [B] fp64 (stays on the device).
    want_msc=True returns (score, msc [129] / [B, 129] fp64): the coherence the score is the weighted sum of."""
    _check_levels(num_levels)
    (c, e), one_d = to_device_batch(clean_signal, enhanced_signal)
    B, L = c.shape
    if L < 1:
        out = (torch.zeros(B, device=c.device, dtype=torch.float64), torch.zeros(B, ops.CSII_BINS, device=c.device, dtype=torch.float64))
    else:
        seg = Fn.PackedSegments(np.full(B, 1 + L // config.HOP_SIZE), np.full(B, L))
        out = csii_packed(c.reshape(-1), e.reshape(-1), seg, fs, True)
    score, msc = (float(out[0][0]), out[1][0]) if one_d else out
    return (score, msc) if want_msc else score
