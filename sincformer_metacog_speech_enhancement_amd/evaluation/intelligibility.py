"""CSII and NCM over a RAGGED set (the calling convention of packed.compute_metrics_packed, which keeps its own three measures):
CSII in one packed pass over the set, NCM in groups of utterances whose filtered planes stay under a byte budget."""
import numpy as np
import torch

from .. import config, functional as Fn, ops
from . import csii, ncm
from .packed import trim_pairs

INTELLIGIBILITY_METRICS = ("csii", "ncm")


def compute_intelligibility_packed(clean, enhanced, seg=None, fs=None, metrics=INTELLIGIBILITY_METRICS, gfb=None, num_levels=3,
                                   group_bytes=None):
    """clean, enhanced: [sum_L] fp32 device tensors holding the utterances of `seg` (a functional.PackedSegments that carries
    `lengths`) back to back - or two lists of 1-D arrays / tensors, then each pair is cut to its shorter member and the set is
    packed once.  Returns {metric: [B] fp64 device tensor}, every utterance scored - bit for bit - as compute_csii / compute_ncm
    score it alone: fewer samples than one 16 ms frame gives CSII 0.0, fewer than 64 NCM 0.0.
    group_bytes: the most filtered-plane bytes (2 x C x 4 per padded sample) NCM holds at a time; default ncm.GROUP_BYTES."""
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in INTELLIGIBILITY_METRICS]
    if bad or not metrics:
        raise ValueError("metrics %r: choose from %r" % (metrics, INTELLIGIBILITY_METRICS))
    if "csii" in metrics:
        csii._check_levels(num_levels)
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP metrics need an MI355X (no CPU fallback)")
    if seg is None:
        c, e = trim_pairs(clean, enhanced)
        if not c:
            return {m: torch.zeros(0, device="cuda", dtype=torch.float64) for m in metrics}
        L = np.asarray([s.size for s in c], dtype=np.int64)
        seg = Fn.PackedSegments(1 + L // config.HOP_SIZE, L)
        stage = torch.empty(2, max(seg.sum_L, 1), dtype=torch.float32, pin_memory=True)
        if seg.sum_L:
            np.concatenate(c, out=stage.numpy()[0, :seg.sum_L])
            np.concatenate(e, out=stage.numpy()[1, :seg.sum_L])
        both = stage.cuda(non_blocking=True)
        clean, enhanced = both[0, :seg.sum_L], both[1, :seg.sum_L]
    if seg.lengths is None:
        raise ValueError("compute_intelligibility_packed: the segments must carry the signal lengths")
    if not torch.is_tensor(clean) or not torch.is_tensor(enhanced):
        raise TypeError("compute_intelligibility_packed: with segments, clean and enhanced are packed device tensors")
    ops._need_dev(clean, enhanced)
    clean, enhanced = clean.detach().float().contiguous(), enhanced.detach().float().contiguous()
    if clean.dim() != 1 or clean.numel() != seg.sum_L or enhanced.shape != clean.shape:
        raise RuntimeError("compute_intelligibility_packed: %s / %s samples, the segments describe [%d]" % (
            tuple(clean.shape), tuple(enhanced.shape), seg.sum_L))
    dev, B = clean.device, seg.B
    out = {}
    if "csii" in metrics:
        out["csii"] = csii.csii_packed(clean, enhanced, seg, fs) if seg.sum_L else torch.zeros(B, device=dev, dtype=torch.float64)
    if "ncm" in metrics:
        bank = gfb or ncm.default_bank(fs)
        score = torch.zeros(B, device=dev, dtype=torch.float64)
        live = np.flatnonzero(seg.lengths >= ncm.MIN_LEN)                     # the others score 0.0 and are not filtered
        lens, offs = seg.lengths[live], seg.sample_offsets[live]
        live_d = torch.from_numpy(live).to(dev)
        both = torch.stack([clean, enhanced])
        for a, b in ncm.plan_groups(lens, bank.num_channels, group_bytes):
            Lg = int(lens[a:b].max())
            meta = torch.from_numpy(np.stack([offs[a:b], lens[a:b]])).to(dev)
            pos = torch.arange(Lg, device=dev)[None, :]
            inside = pos < meta[1][:, None]
            src = (meta[0][:, None] + pos).clamp_max(seg.sum_L - 1)
            padded = torch.where(inside[None], both[:, src], both.new_zeros(()))          # [2, Bg, Lg], 0 behind each utterance
            score[live_d[a:b]] = ncm.ncm_padded(padded[0], padded[1], lens[a:b], bank)
        out["ncm"] = score
    return {m: out[m] for m in metrics}
