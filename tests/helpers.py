"""Shared test helpers: synthetic state_dicts shaped like the reference's
modules (tests/golden/state_shapes.json, captured from the reference) and
golden loaders.  Test-side only."""
import json
import math
import os
import numpy as np
import torch

from sincformer_metacog_speech_enhancement_amd import synthetic as syn
from oracle import sfm_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "state_shapes.json")) as _fh:
    STATE_TABLES = json.load(_fh)


def gold(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def synth_sd(table, seed, fs=16000, sinc_scale=None, as_torch=True):
    """State dict for reference module `table` filled by synthetic.synth_state_dict."""
    shapes = {k: tuple(v[0]) for k, v in STATE_TABLES[table]["state"].items()}
    keep = None
    sinc_keys = [k for k in shapes if k.split(".")[-1] in ("low_hz_", "band_hz_", "window", "n_")]
    if sinc_keys:
        init = orc.sinc_init(64, 251, fs)
        keep = {k: init[k.split(".")[-1]].numpy() for k in sinc_keys}
    sd = syn.synth_state_dict(shapes, seed, keep=keep, sinc_scale=sinc_scale)
    if as_torch:
        return {k: torch.from_numpy(v) for k, v in sd.items()}
    return sd


def arr(key, shape, seed, scale=1.0):
    return torch.from_numpy(syn.synth_array(key, shape, seed, scale))


def maxerr(a, b):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max())


def rmse(a, b):
    a = torch.as_tensor(np.asarray(a)).double()
    b = torch.as_tensor(np.asarray(b)).double()
    return float(((a - b) ** 2).mean().sqrt())


def metric_cases():
    """(name, fs, clean, enhanced) pairs shared by the generator and the tests: plain noisy pairs at both sample rates,
    a silent stretch (skipped frames), identical signals (upper bound), ragged length, shorter-than-a-frame."""
    cases = []
    for i, (fs, L) in enumerate(((8000, 8000), (16000, 12345), (8000, 3001))):
        noisy, clean = syn.synth_wave(1, L, 120 + i)
        cases.append(("pair%d" % i, fs, clean[0], (0.7 * noisy[0] + 0.3 * clean[0]).astype(np.float32)))
    noisy, clean = syn.synth_wave(1, 6000, 125)
    c = clean[0].copy()
    c[2000:3500] = 0.0
    cases.append(("silence", 8000, c, noisy[0]))
    cases.append(("identical", 8000, clean[0], clean[0].copy()))
    cases.append(("short", 8000, clean[0][:100], noisy[0][:100]))
    return cases


def central_difference_along_gradient(params, objective, eps):
    """objective() -> scalar tensor with grad; returns (|g|, central-difference slope of the objective along g / |g|)"""
    total = objective()
    total.backward()
    params = [p_ for p_ in params if p_.grad is not None]
    gnorm = float(torch.sqrt(sum((p_.grad.double() ** 2).sum() for p_ in params)))
    assert math.isfinite(gnorm) and gnorm > 0
    base = [p_.detach().clone() for p_ in params]
    vals = []
    for sign in (1.0, -1.0):
        with torch.no_grad():
            for p_, b0 in zip(params, base):
                p_.copy_(b0 + sign * eps * p_.grad / gnorm)
        vals.append(float(objective().detach()))
    with torch.no_grad():
        for p_, b0 in zip(params, base):
            p_.copy_(b0)
    return float(total.detach()), gnorm, (vals[0] - vals[1]) / (2 * eps)


# ---------------------------------------------------------------------------
# Conformer widths pinned against the oracle (tests/test_widths_gpu.py).  One row per route it is there to exercise;
# tests/test_host_logic.py checks on CPU that the bounds below separate plausible wrong answers at every row.
# train_KS / train_BT: the training-mode check's kernel size and batch x frames (sfm_dwconv_wgrad takes k 7 / 31; w512 trains
# on fewer frames; w256h8 keeps M >= 4096 so the training forward's lin256 routing is covered).
# ---------------------------------------------------------------------------
WIDTH_ROWS = [
    dict(id="w128", D=128, H=2, FF=512, KS=31, BT=(2, 200), train_KS=31, train_BT=(2, 200),
         route="MFMA attention at D 128; un-fused FFN; folded dwconv C 128"),
    dict(id="w192", D=192, H=4, FF=768, KS=15, BT=(2, 150), train_KS=7, train_BT=(2, 150),
         route="generic attention hd 48; LayerNorm D 192; dwconv_bn_swish C 192 k 15"),
    dict(id="w256h8", D=256, H=8, FF=1024, KS=31, BT=(2, 2100), train_KS=31, train_BT=(2, 2100),
         route="ln+lin256, lin256 and ffn_fused_ln with generic attention (hd 32) at T 2100"),
    dict(id="w256h2", D=256, H=2, FF=1000, KS=31, BT=(3, 100), train_KS=31, train_BT=(3, 100),
         route="generic attention hd 128; FF % 64 != 0: un-fused FFN at D 256"),
    dict(id="w384", D=384, H=6, FF=1536, KS=31, BT=(2, 300), train_KS=31, train_BT=(2, 300),
         route="ln_linear16 un-fused fallback at D 384; MFMA attention H 6; LayerNorm D 384; dwconv_bn_swish C 384"),
    dict(id="w512", D=512, H=8, FF=2048, KS=31, BT=(16, 512), train_KS=31, train_BT=(2, 256),
         route="LayerNorm D 512; folded dwconv C 512; pipelined attention kernel at H 8 (B*H*ceil(T/512) = 128)"),
    dict(id="w512h4", D=512, H=4, FF=2048, KS=7, BT=(2, 64), train_KS=7, train_BT=(2, 64),
         route="generic attention hd 128 at D 512; folded dwconv k 7"),
]
# eval: relative RMSE of each module's output vs the float64 oracle.  fp16 as test_conformer_block_full_vs_golden; mixed / bf16
# tighter than its 1.5e-2: measured on the MI355X at most 1.9e-3 (mixed) / 3.7e-3 (bf16) over every row and part (fp16 4.7e-4)
WIDTH_EVAL_TOL = {"fp16": 2e-3, "mixed": 1e-2, "bf16": 1e-2}
WIDTH_QSCALE = 3.0          # Q rows of in_proj scaled up: peaked softmax rows, so the attention branch is far from a time average


def width_block_state(D, H, FF, KS, seed=7):
    """float32 state dict of ConformerBlock(D, H, FF, KS) filled by synthetic.synth_state_dict from the module's own shapes"""
    from sincformer_metacog_speech_enhancement_amd.models.conformer import ConformerBlock
    shapes = {k: tuple(v.shape) for k, v in ConformerBlock(D, H, FF, KS, 0.0).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, seed).items()}
    sd["mhsa.attention.in_proj_weight"][:D] *= WIDTH_QSCALE
    return sd


def width_input(B, T, D, seed=8):
    """[B, T, D] float32 with per-channel scales 0.7 .. 1.5 and offsets -0.3 .. 0.3 (so row statistics over a subset of the
    columns differ from those over all of them)"""
    z = torch.from_numpy(syn.synth_array("width_x", (B, T, D), seed))
    return (z * torch.linspace(0.7, 1.5, D) + torch.linspace(-0.3, 0.3, D)).float().contiguous()


def rel_rmse(got, ref):
    ref = torch.as_tensor(np.asarray(ref)).double()
    return rmse(got, ref) / max(float(ref.pow(2).mean().sqrt()), 1e-30)
