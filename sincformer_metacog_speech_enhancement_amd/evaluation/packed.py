"""The three measures of the reference's evaluate loop (main.py:315-359: compute_stoi, compute_pesq, compute_ssnr per test
file) for a RAGGED set in packed passes: the utterances back to back, each measure over its own framing of every utterance,
per-utterance scores out.  No padding, no per-utterance launch, no host synchronisation."""
import numpy as np
import torch

from .. import config, functional as Fn, ops
from .pesq_eval import pesq_framing, pesq_from_lsd
from . import stoi_taal
from .stoi import _dft_operand

METRICS = ("stoi", "pesq", "ssnr")
ALL_METRICS = METRICS + stoi_taal.TAAL_METRICS      # "stoi" is the reference's fallback, "stoi_taal" / "estoi" the standard measure


def metric_framings(fs=None):
    """{metric: (frame, hop)}: SSNR on the model's framing whatever fs (the reference calls compute_ssnr(clean, enhanced, fs) and
    fs is not used there), STOI 25.6 ms and the PESQ fallback 32 ms frames of fs, half overlap"""
    fs = fs or config.SAMPLE_RATE
    stoi = int(0.0256 * fs)
    return {"ssnr": (config.FRAME_SIZE, config.HOP_SIZE), "stoi": (stoi, stoi // 2), "pesq": pesq_framing(fs)}


def _check_metrics(metrics):
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in ALL_METRICS]
    if bad or not metrics:
        raise ValueError("metrics %r: choose from %r" % (metrics, ALL_METRICS))
    return metrics


def _as_1d(s):
    return np.ascontiguousarray(s.detach().cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1)


def trim_pairs(first, second):
    """two lists of 1-D arrays / tensors -> two lists of float32 numpy arrays, each pair cut to its shorter member
    (evaluation/ssnr.py:50-52).  Host only."""
    first, second = list(first), list(second)
    if len(first) != len(second):
        raise ValueError("%d and %d signals: the two lists must pair up" % (len(first), len(second)))
    a, b = [], []
    for x, y in zip(first, second):
        x, y = _as_1d(x), _as_1d(y)
        n = min(x.size, y.size)
        a.append(x[:n])
        b.append(y[:n])
    return a, b


def plan_evaluation(clean_signals, noisy_signals, n_fft=None, hop=None, max_frames=None):
    """host part of ConformerPipeline.evaluate_batch (no GPU needed): pairs cut to their shorter member, the lengths the
    enhancer refuses raised as functional.packed_segments raises them, and the packed passes.  -> (clean, noisy, passes)"""
    clean, noisy = trim_pairs(clean_signals, noisy_signals)
    passes = Fn.packed_segments([s.size for s in noisy], n_fft or config.FFT_SIZE, hop or config.HOP_SIZE, max_frames)
    return clean, noisy, passes


def _spectra(wave, W, samp_off, tab, B, frame, hop):
    F = frame // 2 + 1
    re = torch.empty(tab["sum"], F, device=wave.device, dtype=torch.float32)
    im = torch.empty(tab["sum"], F, device=wave.device, dtype=torch.float32)
    ops.framed_gemm_varlen(wave, W, re, samp_off, tab["frame_off"], B=B, sum_T=tab["sum"], hop=hop, padl=0, K=frame, N=2 * F,
                           ldm=F, mode=0, out2=im, nsplit=F)
    return re, im


def pack_pairs(clean, enhanced, seg, who):
    """the calling convention of the packed measures: with `seg`, clean / enhanced are [sum_L] device tensors (checked, made fp32
    and contiguous); without, two lists of 1-D signals that are cut pairwise and packed once through pinned memory.
    -> (clean, enhanced, seg), or (None, None, None) for two empty lists"""
    if seg is None:
        c, e = trim_pairs(clean, enhanced)
        if not c:
            return None, None, None
        L = np.asarray([s.size for s in c], dtype=np.int64)
        seg = Fn.PackedSegments(1 + L // config.HOP_SIZE, L)
        stage = torch.empty(2, max(seg.sum_L, 1), dtype=torch.float32, pin_memory=True)
        np.concatenate(c, out=stage.numpy()[0, :seg.sum_L])
        np.concatenate(e, out=stage.numpy()[1, :seg.sum_L])
        both = stage.cuda(non_blocking=True)
        clean, enhanced = both[0, :seg.sum_L], both[1, :seg.sum_L]
    if seg.lengths is None:
        raise ValueError("%s: the segments must carry the signal lengths" % who)
    ops._need_dev(clean, enhanced)
    clean, enhanced = clean.float().contiguous(), enhanced.float().contiguous()
    if clean.dim() != 1 or clean.numel() != seg.sum_L or enhanced.shape != clean.shape:
        raise RuntimeError("%s: %s / %s samples, the segments describe [%d]" % (
            who, tuple(clean.shape), tuple(enhanced.shape), seg.sum_L))
    return clean, enhanced, seg


def compute_metrics_packed(clean, enhanced, seg=None, fs=None, metrics=METRICS, clean_spectra=None):
    """clean, enhanced: [sum_L] fp32 device tensors holding the utterances of `seg` (a functional.PackedSegments that carries
    `lengths`) back to back - or two lists of 1-D arrays / tensors, then each pair is cut to its shorter member and the set is
    packed once.  Returns {metric: [B] fp64 device tensor} for the requested metrics, every utterance scored as
    compute_stoi / compute_pesq / compute_ssnr score it alone: fewer samples than one frame gives SSNR 0.0, STOI 0.0, PESQ 1.0,
    no non-silent frame gives SSNR 0.0.  Nothing in here waits for the device.
    clean_spectra: a dict the caller keeps between calls that score different signals against the SAME clean pack; the clean
    spectra are then computed once."""
    metrics = _check_metrics(metrics)
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP metrics need an MI355X (no CPU fallback)")
    clean, enhanced, seg = pack_pairs(clean, enhanced, seg, "compute_metrics_packed")
    if seg is None:
        return {m: torch.zeros(0, device="cuda", dtype=torch.float64) for m in metrics}
    dev, B = clean.device, seg.B
    fr = metric_framings(fs)
    tabs = seg.metric_tables(dev, tuple(fr[m] for m in metrics if m in fr))
    samp_off = seg.tables(dev)["samp_off"]
    out = {}
    taal = tuple(m for m in metrics if m in stoi_taal.TAAL_METRICS)
    if taal:                                                   # one pass serves both measures: they share everything but the segments
        out.update(stoi_taal.score_packed(clean, enhanced, seg, fs, taal, clean_spectra))
    for m in metrics:
        if m in out:
            continue
        frame, hop = fr[m]
        tab = tabs[fr[m]]
        if tab["sum"] == 0:                                   # no utterance reaches one frame of this measure
            out[m] = torch.full((B,), 1.0 if m == "pesq" else 0.0, device=dev, dtype=torch.float64)
            continue
        if m == "ssnr":
            acc = ops.ssnr_frames_varlen(clean, enhanced, samp_off, tab["frame_off"], B, tab["sum"], frame, hop)
            out[m] = torch.where(acc[:, 1] > 0, acc[:, 0] / acc[:, 1].clamp_min(1.0), torch.zeros_like(acc[:, 0]))
            continue
        W = _dft_operand(frame, dev, "hann" if m == "stoi" else "rect")
        cs = None if clean_spectra is None else clean_spectra.get((m, frame, hop))
        if cs is None:
            cs = _spectra(clean, W, samp_off, tab, B, frame, hop)
            if clean_spectra is not None:
                clean_spectra[(m, frame, hop)] = cs
        es = _spectra(enhanced, W, samp_off, tab, B, frame, hop)
        n = tab["counts"].double()
        some = n > 0
        if m == "stoi":
            S = ops.wave_moments_varlen(enhanced, clean, samp_off, B, int(seg.lengths.max()))   # {., ., sum e^2, sum c^2, .}
            Ls = (samp_off[1:] - samp_off[:-1]).double().clamp_min(1.0)
            sc = (1.0 / (torch.sqrt(S[:, 3] / Ls) + 1e-10)).contiguous()
            se = (1.0 / (torch.sqrt(S[:, 2] / Ls) + 1e-10)).contiguous()
            acc = ops.stoi_frames_varlen(cs[0], cs[1], es[0], es[1], sc, se, tab["frame_off"], B)
            out[m] = torch.where(some, (acc / n.clamp_min(1.0)).clamp(0.0, 1.0), torch.zeros_like(acc))
        else:
            acc = ops.lsd_frames_varlen(cs[0], cs[1], es[0], es[1], tab["frame_off"], B)
            out[m] = torch.where(some, pesq_from_lsd(acc, n.clamp_min(1.0)), torch.ones_like(acc))
    return {m: out[m] for m in metrics}
