"""STOI of Taal et al. (2011) and its extended form ESTOI (Jensen & Taal 2016) on the device: the measure the reference's
evaluation/stoi.py:46-50 computes when pystoi is installed (its requirements.txt lists it; `extended` is config.STOI_EXTENDED).
compute_stoi in stoi.py stays the reference's FALLBACK (_stoi_simplified); these entry points are the standard measure.

Per pair, cut to its shorter member: (0) both signals to 10 kHz through a polyphase FIR, (1) the frames of 256 samples at hop 128
whose windowed CLEAN energy lies within 40 dB of the loudest are kept and both signals rebuilt as the overlap-add of their own kept
frames, (2) 512-point spectra of the rebuilt signals' frames but the last, (3) 15 one-third-octave bands from 150 Hz, (4) fewer than
30 spectral frames -> 1e-5, (5) the 30-frame segment correlations: clipped (STOI) or row- and column-normalised (ESTOI).

The host designs operands and tables in float64 with numpy (no scipy); the device work is csrc/stoi.hip: operands and stored
results are fp32, every sum is fp64 (the resampler's taps on the vector pipe, the DFT on the fp64 matrix instruction).  Nothing here waits for the device: an utterance's kept-frame count stays there
and every table is sized for all frames kept.

The measure as a training objective: stoi_taal_scores is compute_stoi_taal for a [B, L] batch with a graph behind the enhanced
signal (train.StoiTaalFunction, training.TaalSTOILoss).  The kept list and K belong to the clean signal, so the gradient is exact;
gradient_flat walks segments, bands and overlap-add back (csrc/stoi_bwd.hip) and applies the resampler's adjoint, which is the
resampling kernel itself with up and down exchanged (resample_adjoint_operand).  batch_plan keeps plan and uploaded tables per
batch shape: a repeated shape costs no host-device copy and no synchronisation.

The resampler: pystoi resamples with its own Octave-style filter; the default filter of scipy.signal.resample_poly (Kaiser 5.0
windowed sinc, 2 * 10 * max(up, down) + 1 taps, zero phase, zeros beyond both ends) stands in for it here.  The difference
between the two on the score is unmeasured."""
import math

import numpy as np
import torch

from .. import config, ops
from ._common import to_device_batch

RATES = (8000, 10000, 16000)
FS, FRAME, HOP, NFFT, BANDS, SEG = ops.STOI_FS, ops.STOI_FRAME, ops.STOI_HOP, ops.STOI_NFFT, ops.STOI_BANDS, ops.STOI_SEG
MIN_FREQ = 150.0
TOO_SHORT = 1e-5
TAAL_METRICS = ("stoi_taal", "estoi")

_operands = {}
_plans = {}
PLAN_CACHE = 64                 # batch shapes whose plan and uploaded tables are kept (batch_plan)


# ---- host design (float64, numpy only) ----
def check_rate(fs):
    fs = int(fs or config.SAMPLE_RATE)
    if fs not in RATES:
        raise NotImplementedError("STOI (Taal): sample rate %d Hz; the supported rates are %r" % (fs, RATES))
    return fs


def rate_ratio(fs):
    """(up, down) of the conversion fs -> 10 kHz"""
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def resample_taps(up, down):
    """float64 [2 * 10 * max(up, down) + 1]: the filter of scipy.signal.resample_poly(x, up, down) with its defaults - firwin's
    windowed sinc (cut-off 1 / max(up, down) of Nyquist, Kaiser 5.0), unit DC gain, times up"""
    rate = max(up, down)
    if rate > ops.STOI_MAX_RATE:
        raise NotImplementedError("STOI (Taal): up %d / down %d beyond %d" % (up, down, ops.STOI_MAX_RATE))
    half = ops.STOI_TAP_HALF * rate
    m = np.arange(2 * half + 1, dtype=np.float64) - half
    fc = 1.0 / rate
    h = fc * np.sinc(fc * m) * np.kaiser(2 * half + 1, 5.0)
    return h / h.sum() * up


def resample_operand(up, down):
    """(W float64 [K, up], padl): output sample t * up + p of a signal x is sum_k x[t * down + k - padl] W[k, p], zeros beyond both
    ends of x - the polyphase form of y[n] = sum_m x[m] h[n * down - m * up + half] (resample_poly's zero-phase alignment)"""
    h = resample_taps(up, down)
    half = (h.size - 1) // 2
    j_min = -(half // up)
    j_max = ((up - 1) * down + half) // up
    K, padl = j_max - j_min + 1, -j_min
    W = np.zeros((K, up))
    for p in range(up):
        for k in range(K):
            i = p * down - (k - padl) * up + half
            if 0 <= i < h.size:
                W[k, p] = h[i]
    return W, padl


def resample_adjoint_operand(up, down):
    """(W float64 [K, down], padl) of the ADJOINT of the conversion that resample_operand(up, down) states: with y = R x,
    (R^T g)[t * down + p] = sum_k g[t * up + k - padl] W[k, p], zeros beyond both ends of g - dx[m] = sum_n dy[n] h[n down - m up + half],
    the same polyphase form with up and down exchanged and the forward's own taps"""
    h = resample_taps(up, down)
    half = (h.size - 1) // 2
    j_min = -(half // down)
    j_max = ((down - 1) * up + half) // down
    K, padl = j_max - j_min + 1, -j_min
    W = np.zeros((K, down))
    for p in range(down):
        for k in range(K):
            i = (k - padl) * down - p * up + half
            if 0 <= i < h.size:
                W[k, p] = h[i]
    return W, padl


def resampled_lengths(lengths, fs):
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    up, down = rate_ratio(fs)
    return L if int(fs) == FS else -(-L * up // down)


def window():
    return np.hanning(FRAME + 2)[1:-1]


def band_edges():
    """int [16]: band j sums the bins [e[j], e[j + 1]) - centres 150 * 2^(j/3), edges the geometric means of neighbouring centres
    snapped to the nearest bin of linspace(0, 10000, 513)[:257]"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(BANDS, dtype=np.float64)
    cf = MIN_FREQ * 2.0 ** (k / 3.0)
    lo = np.sqrt(cf * MIN_FREQ * 2.0 ** ((k - 1) / 3.0))
    hi = np.sqrt(cf * MIN_FREQ * 2.0 ** ((k + 1) / 3.0))
    a = [int(np.argmin((f - x) ** 2)) for x in lo]
    b = [int(np.argmin((f - x) ** 2)) for x in hi]
    if a[1:] != b[:-1] or a[0] != ops.STOI_FIRST_BIN or b[-1] != ops.STOI_LAST_BIN + 1:
        raise AssertionError("the band table no longer matches SFM_STOI_FIRST_BIN / SFM_STOI_LAST_BIN")
    return np.asarray(a + [b[-1]], dtype=np.int64)


def dft_operand():
    """float64 [256, 432]: column c < 212 = cos(2 pi n (c + 7) / 512), column 212 + c = -sin(.), zero beyond 424"""
    n = np.arange(FRAME, dtype=np.float64)[:, None]
    f = np.arange(ops.STOI_FIRST_BIN, ops.STOI_LAST_BIN + 1, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * ((n * f) % NFFT) / NFFT
    D = np.zeros((FRAME, ops.STOI_DFT_COLS))
    D[:, :ops.STOI_NBIN] = np.cos(ang)
    D[:, ops.STOI_NBIN:2 * ops.STOI_NBIN] = -np.sin(ang)
    return D


def plan_tables(lengths, fs, sample_offsets=None):
    """host tables of one pass over utterances of `lengths` samples at fs (no GPU needed; all frames kept is the upper bound every
    size is planned for).  sample_offsets [B] or [B + 1]: where each utterance starts in the flat signal (default: back to back).
    -> dict: in_off, in_len [B] (the signals at fs), sig_off, sig_len [B] (the 10 kHz signals: the same at 10 kHz, else back to
    back), frame_off [B + 1], frames [B], tiles [n, 2] = (utterance, tile of 16 spectral frames), spec_rows, segments, sum_frames,
    n_samples (at 10 kHz), n_in"""
    fs = check_rate(fs)
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    B = L.size
    if B == 0 or int(L.min()) < 0:
        raise ValueError("plan_tables: %d utterances, shortest %s" % (B, L.min() if B else None))
    up, down = rate_ratio(fs)
    Lr = resampled_lengths(L, fs)
    in_off = np.concatenate([[0], np.cumsum(L)])[:B] if sample_offsets is None else np.asarray(sample_offsets, dtype=np.int64)[:B]
    sig_off = in_off if fs == FS else np.concatenate([[0], np.cumsum(Lr)])[:B]
    frames = np.where(Lr >= FRAME, (Lr - FRAME) // HOP + 1, 0)
    frame_off = np.concatenate([[0], np.cumsum(frames)])
    spec = np.maximum(frames - 1, 0)
    nt = -(-spec // ops.STOI_ROW_TILE)
    utt = np.repeat(np.arange(B), nt)
    tile = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    tiles = np.ascontiguousarray(np.stack([utt, tile], axis=1), dtype=np.int64)
    top = max(int((in_off + L).max()), int((sig_off + Lr).max()), int(frame_off[-1]))
    if top >= 2 ** 31:
        raise ValueError("a packed pass is indexed with int32: %d samples / rows" % top)
    return {"B": B, "fs": fs, "up": up, "down": down, "in_off": in_off, "in_len": L, "sig_off": sig_off, "sig_len": Lr,
            "frame_off": frame_off, "frames": frames, "tiles": tiles, "spec_rows": int(spec.sum()),
            "segments": int(np.maximum(spec - (SEG - 1), 0).sum()), "sum_frames": int(frame_off[-1]), "n_samples": int(Lr.sum()),
            "n_in": int(L.sum())}


# ---- device ----
def _upload(plan, dev):
    """the plan's int32 tables in ONE copy"""
    B = plan["B"]
    parts = [plan["in_off"], plan["in_len"], plan["sig_off"], plan["sig_len"], plan["frame_off"], plan["tiles"].reshape(-1)]
    flat = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(dev)
    cut = np.cumsum([0] + [p.size for p in parts])
    t = {k: flat[cut[i]:cut[i + 1]] for i, k in enumerate(("in_off", "in_len", "sig_off", "sig_len", "frame_off", "tiles"))}
    t["tiles"] = t["tiles"].view(-1, 2)
    assert t["frame_off"].numel() == B + 1
    return t


def _device_operands(dev, fs):
    key = (str(dev), fs)
    o = _operands.get(key)
    if o is None:
        base = _operands.get(str(dev))
        if base is None:
            base = _operands[str(dev)] = {
                "win": torch.from_numpy(window().astype(np.float32)).to(dev),
                "dft": torch.from_numpy(dft_operand().astype(np.float32)).to(dev).contiguous()}
        o = dict(base)
        if fs != FS:
            W, padl = resample_operand(*rate_ratio(fs))
            o["taps"], o["padl"] = torch.from_numpy(W.astype(np.float32)).to(dev).contiguous(), padl
        _operands[key] = o
    return o


def _resample(sig, plan, tabs, op):
    if plan["fs"] == FS:
        return sig
    return ops.stoi_resample(sig, op["taps"], tabs["in_off"], tabs["in_len"], tabs["sig_off"], tabs["sig_len"], plan["B"],
                             plan["n_samples"], int(plan["sig_len"].max()), plan["n_in"], plan["up"], plan["down"], op["padl"])


def _adjoint_operands(dev, fs):
    """the forward's operands and, made on first use, what the gradient adds: the transposed DFT matrix and the adjoint taps"""
    o = _device_operands(dev, fs)
    if "dft_t" not in o:
        o["dft_t"] = torch.from_numpy(np.ascontiguousarray(dft_operand().astype(np.float32).T)).to(dev)
        if fs != FS:
            W, padl = resample_adjoint_operand(*rate_ratio(fs))
            o["taps_t"], o["padl_t"] = torch.from_numpy(W.astype(np.float32)).to(dev).contiguous(), padl
    return o


def analyse_flat(clean, enhanced, plan, tabs, clean_state=None):
    """steps 0-3 of score_flat (plan["sum_frames"] > 0) -> {"re": the enhanced signal at 10 kHz, "src", "kept": the kept list,
    "xb", "yb": the band rows of the clean and the enhanced signal} - what the segment kernel reads and the gradient keeps"""
    B = plan["B"]
    op = _device_operands(clean.device, plan["fs"])
    args = (op["win"], op["dft"], tabs["sig_off"], tabs["frame_off"])
    cs = None if clean_state is None else clean_state.get(("stoi_taal", plan["fs"]))
    re = _resample(enhanced, plan, tabs, op)
    if cs is None:
        rc = _resample(clean, plan, tabs, op)
        src, kept, _ = ops.stoi_keep(rc, op["win"], tabs["sig_off"], tabs["sig_len"], tabs["frame_off"], B, plan["sum_frames"],
                                     plan["n_samples"])
        xb, yb = ops.stoi_bands((rc, re), *args, src, kept, tabs["tiles"], plan["sum_frames"], plan["spec_rows"], plan["n_samples"])
        if clean_state is not None:
            clean_state[("stoi_taal", plan["fs"])] = {"src": src, "kept": kept, "bands": xb}
    else:
        src, kept, xb = cs["src"], cs["kept"], cs["bands"]
        yb, = ops.stoi_bands((re,), *args, src, kept, tabs["tiles"], plan["sum_frames"], plan["spec_rows"], plan["n_samples"])
    return {"re": re, "src": src, "kept": kept, "xb": xb, "yb": yb}


def score_flat(clean, enhanced, plan, tabs, measures, clean_state=None):
    """clean, enhanced: flat fp32 device signals at plan["fs"], utterance u = plan["in_len"][u] samples from plan["in_off"][u] (nothing
    beyond them is read); tabs = the uploaded plan.  -> {measure: [B] fp64} for measures out of TAAL_METRICS.
    clean_state: a dict that keeps what later calls on the same clean pack need of the clean side - the kept list ("src", "kept")
    and the band rows ("bands"), so the clean signal is neither resampled nor analysed again."""
    dev, B = clean.device, plan["B"]
    if plan["sum_frames"] == 0:
        return {m: torch.full((B,), TOO_SHORT, device=dev, dtype=torch.float64) for m in measures}
    a = analyse_flat(clean, enhanced, plan, tabs, clean_state)
    return {m: ops.stoi_segments(a["xb"], a["yb"], tabs["frame_off"], a["kept"], B, m == "estoi", plan["spec_rows"], plan["segments"])
            for m in measures}


def gradient_flat(a, plan, tabs, gscore, extended, row):
    """the gradient of sum_u gscore[u] score[u] by the enhanced signal of a [B, row] batch: a = analyse_flat's result, gscore fp64
    [B] on the device -> fp32 [B * row], every element written, zeros from in_len[u] on.  Segments, bands and overlap-add walked
    back (csrc/stoi_bwd.hip), then the resampler's adjoint: sfm_stoi_resample with resample_adjoint_operand."""
    dev, B, fs = a["re"].device, plan["B"], plan["fs"]
    op = _adjoint_operands(dev, fs)
    dyb = ops.stoi_segments_bwd(a["xb"], a["yb"], tabs["frame_off"], a["kept"], gscore, B, int(plan["frames"].max()), extended,
                                plan["spec_rows"], plan["segments"])
    dfr = ops.stoi_bands_bwd(a["re"], op["win"], op["dft"], op["dft_t"], tabs["sig_off"], tabs["frame_off"], a["src"], a["kept"],
                             tabs["tiles"], dyb, plan["sum_frames"], plan["spec_rows"], plan["n_samples"])
    fold = (dfr, op["win"], tabs["sig_off"], tabs["sig_len"], tabs["frame_off"], a["src"], a["kept"], B)
    if fs == FS:                                              # the 10 kHz signal IS the batch: rows of `row` samples
        return ops.stoi_fold_bwd(*fold, B * row, row, row, plan["sum_frames"])[:B * row]
    d10 = ops.stoi_fold_bwd(*fold, plan["n_samples"], int(plan["sig_len"].max()), 0, plan["sum_frames"])
    ragged = int(plan["in_len"].min()) < row
    out = (torch.zeros if ragged else torch.empty)(B * row, device=dev, dtype=torch.float32)
    ops.stoi_resample(d10, op["taps_t"], tabs["sig_off"], tabs["sig_len"], tabs["in_off"], tabs["in_len"], B, B * row,
                      int(plan["in_len"].max()), plan["n_samples"], plan["down"], plan["up"], op["padl_t"], out=out)
    return out


def batch_plan(fs, B, L, lengths, dev):
    """(plan, uploaded tables) of a [B, L] batch whose row u holds lengths[u] samples (None: L), kept by (device, fs, B, L, lengths):
    a repeated shape costs neither a host-device copy nor a synchronisation"""
    if lengths is None:
        Lh = (L,) * B
    else:
        Lh = tuple(int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths))
        if len(Lh) != B or (B and (min(Lh) < 0 or max(Lh) > L)):
            raise ValueError("lengths %r for a [%d, %d] batch" % (list(Lh), B, L))
    key = (str(dev), fs, B, L, Lh)
    hit = _plans.get(key)
    if hit is None:
        plan = plan_tables(Lh, fs, np.arange(B, dtype=np.int64) * L)
        if len(_plans) >= PLAN_CACHE:
            _plans.clear()
        hit = _plans[key] = (plan, _upload(plan, dev))
    return hit


def _packed_plan(seg, fs, dev):
    """plan and uploaded tables of a PackedSegments, cached on it like its other tables"""
    key = ("stoi_taal", str(dev), fs)
    hit = seg._tables.get(key)
    if hit is None:
        plan = plan_tables(seg.lengths, fs, seg.sample_offsets)
        hit = seg._tables[key] = (plan, _upload(plan, dev))
    return hit


def score_packed(clean, enhanced, seg, fs, measures, clean_state=None):
    """the packed pass behind compute_stoi_taal_packed and compute_metrics_packed: clean, enhanced [sum_L] fp32 on the device"""
    fs = check_rate(fs)
    plan, tabs = _packed_plan(seg, fs, clean.device)
    return score_flat(clean, enhanced, plan, tabs, measures, clean_state)


def compute_stoi_taal(clean_signal, enhanced_signal, fs=None, extended=False, lengths=None):
    """STOI (extended: ESTOI) of Taal et al.  1-D inputs -> float; [B, L] inputs -> fp64 device tensor [B].  lengths [B]: the
    sample counts of zero-padded rows.  Inputs are numpy arrays or tensors, cut to the shorter of the two."""
    fs = check_rate(fs)
    (c, e), one_d = to_device_batch(clean_signal, enhanced_signal)
    B, L = c.shape
    if lengths is None:
        Lh = np.full(B, L, dtype=np.int64)
    else:
        Lh = np.asarray(lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
        if Lh.size != B or int(Lh.min()) < 0 or int(Lh.max()) > L:
            raise ValueError("compute_stoi_taal: lengths %r for a [%d, %d] batch" % (Lh.tolist(), B, L))
    plan = plan_tables(Lh, fs, np.arange(B, dtype=np.int64) * L)      # (nothing behind a row's length is read)
    m = "estoi" if extended else "stoi_taal"
    out = score_flat(c.reshape(-1), e.reshape(-1), plan, _upload(plan, c.device), (m,))[m]
    return float(out[0]) if one_d else out


def compute_stoi_taal_packed(clean, enhanced, seg=None, fs=None, extended=False, clean_state=None):
    """clean, enhanced: [sum_L] fp32 device tensors holding the utterances of `seg` (a functional.PackedSegments that carries
    `lengths`) back to back - or two lists of 1-D arrays / tensors, then each pair is cut to its shorter member and the set is
    packed once (the convention of compute_metrics_packed).  -> [B] fp64 on the device, every utterance scored - bit for bit -
    as compute_stoi_taal scores it alone.  clean_state (beyond the reference-style signature, optional): a dict the caller keeps
    between calls that score different signals against the SAME clean pack, as compute_metrics_packed's clean_spectra; after a
    call clean_state[("stoi_taal", fs)]["kept"] is the device's int32 [B] count of kept frames."""
    from .packed import pack_pairs
    fs = check_rate(fs)
    m = "estoi" if extended else "stoi_taal"
    clean, enhanced, seg = pack_pairs(clean, enhanced, seg, "compute_stoi_taal_packed")
    if seg is None:
        return torch.zeros(0, device="cuda", dtype=torch.float64)
    return score_packed(clean, enhanced, seg, fs, (m,), clean_state)[m]


def scores_and_kept(enhanced, clean, fs, extended, lengths, name="stoi_taal_scores"):
    """stoi_taal_scores with the device's int32 [B] kept-frame counts beside the scores (training.TaalSTOILoss decides from them
    which utterances count)"""
    from .. import train
    fs = check_rate(fs)
    for t in (enhanced, clean):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("%s: device tensors are needed (there is deliberately no CPU fallback)" % name)
    if enhanced.shape != clean.shape or enhanced.dim() not in (1, 2) or enhanced.dtype != torch.float32 or clean.dtype != torch.float32:
        raise ValueError("%s: two fp32 waveforms [L] or [B, L] of one shape are needed; got %s %s and %s %s"
                         % (name, tuple(enhanced.shape), enhanced.dtype, tuple(clean.shape), clean.dtype))
    B, L = (1, enhanced.shape[0]) if enhanced.dim() == 1 else enhanced.shape
    if B < 1 or L < 1:
        raise ValueError("%s: an empty batch" % name)
    plan, tabs = batch_plan(fs, B, L, lengths, enhanced.device)
    return train.StoiTaalFunction.apply(enhanced, clean, plan, tabs, bool(extended))


def stoi_taal_scores(enhanced, clean, fs=None, extended=False, lengths=None):
    """compute_stoi_taal for a batch with a graph behind `enhanced`: fp32 device waveforms [L] or [B, L] of one shape -> [B] fp64
    on the device, bit for bit compute_stoi_taal's values (the same four kernels); the node is train.StoiTaalFunction, the
    gradient goes to `enhanced` only.  lengths: a host sequence [B], the sample counts of zero-padded rows (nothing behind a
    row's length is read; the gradient there is 0)."""
    return scores_and_kept(enhanced, clean, fs, extended, lengths)[0]
