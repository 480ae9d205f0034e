"""evaluation/pesq_eval.py: the reference calls the pesq package (ITU-T P.862) when it is installed and otherwise its own
simplified measure (_pesq_simplified :51-85), a log-spectral distortion mapped to the PESQ range.  Here it is ALWAYS the
simplified measure, whether or not the pesq package is installed, batched on the device.  It is not P.862 (`mode` is
accepted and ignored, as in the fallback)."""
import torch

from .. import config, ops
from ._common import to_device_batch
from .stoi import _dft_operand


def pesq_framing(fs):
    """(frame, hop) of the fallback: 32 ms frames, half overlap (pesq_eval.py:58-59)"""
    frame = int(0.032 * fs)
    return frame, frame // 2


def pesq_from_lsd(lsd_sum, nframes):
    """clip(4.5 - 0.5 * mean lsd, -0.5, 4.5) (pesq_eval.py:80-85)"""
    return (4.5 - 0.5 * lsd_sum / nframes).clamp(-0.5, 4.5)


def compute_pesq(clean_signal, enhanced_signal, fs=None, mode=None):
    """1-D inputs -> float (the reference's signature); [B, L] inputs -> tensor [B] fp64 (stays on the device).
    The simplified measure of the reference's fallback, never P.862: per 32 ms frame (rectangular window, half overlap)
    sqrt(mean_f (log(|C_f| + 1e-10) - log(|E_f| + 1e-10))^2), averaged over the frames, then 4.5 - 0.5 x that, clipped to
    [-0.5, 4.5]; 1.0 for a signal shorter than one frame."""
    fs = fs or config.SAMPLE_RATE
    (c, e), one_d = to_device_batch(clean_signal, enhanced_signal)
    B, L = c.shape
    frame, hop = pesq_framing(fs)
    nframes = (L - frame) // hop + 1 if L >= frame else 0
    if nframes < 1:
        out = torch.ones(B, device=c.device, dtype=torch.float64)
        return 1.0 if one_d else out
    F = frame // 2 + 1
    W = _dft_operand(frame, c.device, "rect")
    spec = []
    for sig in (c, e):
        re = torch.empty(B, nframes, F, device=c.device, dtype=torch.float32)
        im = torch.empty(B, nframes, F, device=c.device, dtype=torch.float32)
        ops.framed_gemm(sig, W, re, B=B, M=nframes, Ls=L, sig_batch_stride=L, hop=hop, padl=0, K=frame, N=2 * F,
                        o_batch_stride=nframes * F, ldm=F, ldn=1, mode=0, out2=im, nsplit=F)
        spec += [re, im]
    out = pesq_from_lsd(ops.lsd_frames(*spec), nframes)
    return float(out[0]) if one_d else out
