"""Shared cases of the hair-cell tests (tests/test_haircell_*.py, tests/golden/make_golden_features.py): a restatement of
signal_processing/haircell.py in torch that computes in the dtype of its input (float64: every step one IEEE double operation in
the reference's order, so it IS the reference on the same input, bit for bit - tests/test_haircell_host.py pins that to captured
outputs), the inputs and the mutants.  Test-side only.

Inputs are what GammatoneFilterbank.filter returns: the float32 restatement of the FIR bank (gammatone_cases.fir) on the seeded
signals, taken at scale 1 - where x + A stays in the neighbourhood of A = 5, the permeability clamp never acts and the cleft clamp
acts on the first step alone - and at scale 1e4, where the permeability clamp max(x + A, 0) acts on half of the samples and the
cleft clamp max(c + dc, 0) whenever the permeability drops (dt (l + r) = 1.135 > 1 at 8 kHz: without new transmitter a step
takes c below zero)."""
import numpy as np
import torch

import gammatone_cases as gc

FRAME, HOP = 160, 80
SCALES = (1.0, 1e4)
FRAMES_RTOL = 1e-12                  # process_to_frames against the restatement: the reassociation of a 160-term fp64 mean
MUTANTS = ("no s clamp", "no c clamp", "frame sum off by one")
GOLDEN_ROWS = (0, 21, 42, 63)        # rows of the [64, 559] input whose reference outputs tests/golden/g21_haircell.npz keeps
RAGGED_LENGTHS = (1153, 700)

_cache = {}


def params(sample_rate=8000):
    """the reference's constants and steady state, in Python floats, in its order of operations"""
    A, B, g, y, l, r, x, h, M = 5.0, 300.0, 2000.0, 5.05, 2500.0, 6580.0, 66.31, 50000.0, 1.0
    k_ss = g * A / (A + B)
    q0 = M * y * k_ss / (l * k_ss + y * (l + r))
    c0 = q0 * k_ss / y
    w0 = c0 * r / x
    return dict(A=A, B=B, g=g, y=y, l=l, r=r, x=x, h=h, M=M, dt=1.0 / sample_rate, q0=q0, c0=c0, w0=w0)


def inputs(name):
    """fp32 CPU inputs: 'c64' [64, 559] (default bank, case d559), 'b20' [2, 20, 1153] (20-channel bank: case c1153 and a second
    seeded signal).  Cached and shared: do not modify."""
    if name not in _cache:
        if name == "c64":
            _cache[name] = gc.analysis("d559", torch.float32)["y"].contiguous()
        else:
            b = gc.bank("ch20")
            h = gc.taps_of(b, torch.float32)
            _cache[name] = torch.stack([gc.analysis("c1153", torch.float32)["y"], gc.fir(gc.signal(1153, 331, "noise"), h)]).contiguous()
    return _cache[name]


def _clamp(v):
    return torch.where(0 > v, torch.zeros_like(v), v)         # Python's max(v, 0): v unless 0 > v


def haircell(x, sample_rate=8000, mutant=None):
    """x [.., L] -> the firing rate [.., L] in x's dtype, every row one chain; float64 on fp32-valued input = the reference"""
    p = params(sample_rate)
    dt = p["dt"]
    out = torch.empty_like(x)
    q = torch.full(x.shape[:-1], p["q0"], dtype=x.dtype)
    c = torch.full(x.shape[:-1], p["c0"], dtype=x.dtype)
    w = torch.full(x.shape[:-1], p["w0"], dtype=x.dtype)
    for t in range(x.shape[-1]):
        s = x[..., t] + p["A"]
        if mutant != "no s clamp":
            s = _clamp(s)
        k = s / (s + p["B"])
        dq = dt * (p["y"] * (p["M"] - q) + p["x"] * w - k * q)
        q = _clamp(q + dq)
        dc = dt * (k * q - p["l"] * c - p["r"] * c)
        c = c + dc if mutant == "no c clamp" else _clamp(c + dc)
        dw = dt * (p["r"] * c - p["x"] * w)
        w = _clamp(w + dw)
        out[..., t] = p["h"] * c
    return out


def frames(rate, frame=FRAME, hop=HOP, mutant=None):
    """[.., L] -> [.., T]: the mean of each frame"""
    if mutant == "frame sum off by one":
        rate = torch.nn.functional.pad(rate[..., 1:], (0, 1))
    return rate.unfold(-1, frame, hop).mean(-1)


def reference(name, scale, mutant=None):
    """(rate [.., L], frames [.., T]) of inputs(name) * scale in float64.  Cached: do not modify."""
    key = ("ref", name, scale, mutant)
    if key not in _cache:
        x = (inputs(name) * np.float32(scale)).double()
        rate = haircell(x, mutant=mutant if mutant != "frame sum off by one" else None)
        _cache[key] = (rate, frames(rate, mutant=mutant))
    return _cache[key]


def rel_distance(a, b):
    """max |a - b| / max |b|"""
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


def separates(name, mutant, wrong, ref, bound):
    """a wrong form must move the reference by >= 5 x the row's bound (max |err| / max |ref|)"""
    moved = rel_distance(wrong, ref)
    print("MUTANT | %s | %s | moves the reference by %.3e, the bound is %.1e" % (name, mutant, moved, bound))
    assert moved >= 5.0 * bound and moved > 0.0, (name, mutant, moved)
