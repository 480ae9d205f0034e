"""The gradient of STOI / ESTOI (Taal) on the device (csrc/stoi_bwd.hip through evaluation.stoi_taal_scores and
training.TaalSTOILoss) against the float64 autograd restatement of tests/stoi_loss_cases.py: within K = 16 x e32g relative RMSE
and exactly 0 where the float64 gradient is, the constant outcomes, independence of the company in a batch, the cotangent, the
forward bit for bit, the module, and the composition with train.IstftFunction."""
import numpy as np
import pytest
import torch

import stoi_loss_cases as lc
import stoi_taal_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from sincformer_metacog_speech_enhancement_amd import config, train
    from sincformer_metacog_speech_enhancement_amd.evaluation import compute_stoi_taal, stoi_taal_scores
    from sincformer_metacog_speech_enhancement_amd.evaluation import stoi_taal as st
    from sincformer_metacog_speech_enhancement_amd.training import TaalSTOILoss
    return {"config": config, "train": train, "taal": compute_stoi_taal, "scores": stoi_taal_scores, "st": st, "loss": TaalSTOILoss}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grad_of(pkg, c, e, fs, ext, lengths=None, weights=None):
    """(scores [B] fp64, gradient like e, float32) on the device, both as numpy"""
    E = dev(e).requires_grad_(True)
    s = pkg["scores"](E, dev(c), fs, ext, lengths)
    assert s.dtype == torch.float64 and s.shape == (1 if e.ndim == 1 else e.shape[0],)
    (s.sum() if weights is None else (s * weights).sum()).backward()
    assert E.grad.dtype == torch.float32 and E.grad.shape == E.shape
    return s.detach().cpu().numpy(), E.grad.cpu().numpy()


# ---- 1. the gradient within its bound ----
@pytest.mark.parametrize("ext", sc.MEASURES)
@pytest.mark.parametrize("num", lc.GRAD_CASES + ("long",))
def test_gradient_within_its_bound(pkg, num, ext):
    """"long": 126 band rows - four row blocks of the segment backward, two stages of segments in a block, rows that wrap its rings"""
    if num == "long":
        (c, e), fs, name, fwd = lc.long_pair(), lc.LONG[1], "long", lc.evaluated()[("long", ext)]["forward"]
    else:
        cs = lc.case(num)
        (c, e), fs, name, fwd = sc.case_pair(cs), cs[1], "case %d" % num, sc.evaluated()[(num, ext)]
    s, g = grad_of(pkg, c, e, fs, ext)
    sc.check("%s %s value" % (name, "estoi" if ext else "stoi"), s[0], fwd)
    lc.check("%s %s gradient" % (name, "estoi" if ext else "stoi"), g, lc.evaluated()[(num, ext)])


# ---- 2. constant outcomes ----
@pytest.mark.parametrize("ext", sc.MEASURES)
def test_constant_outcomes(pkg, ext):
    pairs = [sc.case_pair(lc.case(n)) + (lc.case(n)[1],) for n in lc.CONSTANT_CASES]
    pairs += [sc.pair(L, fs) + (fs,) for fs, L in sc.ONE_FRAME + sc.TWO_FRAMES]
    for c, e, fs in pairs:
        s, g = grad_of(pkg, c, e, fs, ext)
        assert s[0] == 1e-5 and not g.any() and np.isfinite(g).all(), (fs, len(e))
    cs = lc.case(12)                                         # a clean signal of exact zeros
    c, e = sc.case_pair(cs)
    s, g = grad_of(pkg, c, e, cs[1], ext)
    assert np.isfinite(s).all() and np.isfinite(g).all() and not g.any()
    c, e = sc.case_pair(lc.case(6))                          # an enhanced signal of exact zeros
    s, g = grad_of(pkg, c, np.zeros_like(e), 16000, ext)
    assert np.isfinite(s).all() and np.isfinite(g).all() and not g.any()


@pytest.mark.parametrize("ext", sc.MEASURES)
def test_silent_stretch_in_the_enhanced_signal(pkg, ext):
    c, e = lc.silent_pair()
    s, g = grad_of(pkg, c, e, lc.SILENT[1], ext)
    row = lc.evaluated()[("silent", ext)]
    assert np.isfinite(s).all()
    lc.check("silent stretch %s gradient" % ("estoi" if ext else "stoi"), g, row)


# ---- 3. independence of the company ----
# (only the zero-padded [B, L] batch with lengths: the gradient has no packed - ragged, back to back - form, a known gap)
BATCHES = {16000: (7, 11, "long", 6, 8), 10000: (3, 1, 4), 8000: (10, (8000, 300))}


@pytest.mark.parametrize("fs", sorted(BATCHES))
def test_batch_rows_equal_the_utterances_alone_bit_for_bit(pkg, fs):
    pairs = [lc.long_pair() if m == "long" else sc.pair(m[1], m[0]) if isinstance(m, tuple) else sc.case_pair(lc.case(m))
             for m in BATCHES[fs]]
    lengths = [len(e) for _, e in pairs]
    L = max(lengths) + 37
    C, E = np.full((len(pairs), L), np.nan, dtype=np.float32), np.full((len(pairs), L), np.nan, dtype=np.float32)
    for u, (c, e) in enumerate(pairs):
        C[u, :len(c)], E[u, :len(e)] = c, e
    for ext in sc.MEASURES:
        s, g = grad_of(pkg, C, E, fs, ext, lengths)
        s2, g2 = grad_of(pkg, C, E, fs, ext, np.asarray(lengths))
        assert np.array_equal(s, s2) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))      # run to run
        for u, (c, e) in enumerate(pairs):
            s1, g1 = grad_of(pkg, c, e, fs, ext)
            assert s1[0] == s[u], (fs, u, ext)
            assert np.array_equal(g1.view(np.uint32), g[u, :lengths[u]].view(np.uint32)), (fs, u, ext)
            assert not g[u, lengths[u]:].any() and np.isfinite(g[u]).all(), (fs, u, ext)


# ---- 4. the cotangent ----
@pytest.mark.parametrize("ext", sc.MEASURES)
def test_cotangent_is_linear_and_a_zero_weight_gives_zeros(pkg, ext):
    pairs = [sc.case_pair(lc.case(n)) for n in (6, 7, 8)]
    lengths = [len(e) for _, e in pairs]
    C, E = np.zeros((3, max(lengths)), dtype=np.float32), np.zeros((3, max(lengths)), dtype=np.float32)
    for u, (c, e) in enumerate(pairs):
        C[u, :len(c)], E[u, :len(e)] = c, e
    w = [0.5, -2.0, 0.0]
    _, g1 = grad_of(pkg, C, E, 16000, ext, lengths)
    for wdt in (torch.float64, torch.float32):
        _, gw = grad_of(pkg, C, E, 16000, ext, lengths, torch.tensor(w, dtype=wdt).cuda())
        for u in range(2):                                   # four fp32 stores on the way, each within 2^-24 relative
            assert lc.rel_rmse(gw[u], w[u] * g1[u].astype(np.float64)) <= 4 * 2.0 ** -24, (u, wdt)
        assert not gw[2].any()


def test_a_second_backward_and_an_in_place_change(pkg):
    """a retained graph gives the same gradient again (per-term gradient norms to pick the caller's weight), a freed one raises
    and never answers zeros; at 10 kHz the saved signal is the caller's waveform, so changing it in place before the backward raises"""
    cs = lc.case(4)
    c, e = sc.case_pair(cs)
    E = dev(e).requires_grad_(True)
    wav = E * 1.0
    s = pkg["scores"](wav, dev(c), cs[1], True).sum()
    g1, = torch.autograd.grad(s, E, retain_graph=True)
    g2, = torch.autograd.grad(s, E)
    assert torch.equal(g1, g2) and bool(g1.any())
    with pytest.raises(RuntimeError, match="second time"):
        torch.autograd.grad(s, E)
    wav = E * 1.0
    s = pkg["scores"](wav, dev(c), cs[1], True).sum()
    wav.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        s.backward()


# ---- 5. the forward ----
def test_scores_are_compute_stoi_taal_bit_for_bit(pkg):
    for num in (4, 7, 10, 11):
        cs = lc.case(num)
        c, e = sc.case_pair(cs)
        for ext in sc.MEASURES:
            got = pkg["scores"](dev(e), dev(c), cs[1], ext)
            want = pkg["taal"](c, e, fs=cs[1], extended=ext)
            assert got.shape == (1,) and float(got[0]) == want, (num, ext)
    pairs = [sc.case_pair(lc.case(n)) for n in (6, 11, 8)]
    lengths = [len(e) for _, e in pairs]
    C, E = np.zeros((3, 9601), dtype=np.float32), np.zeros((3, 9601), dtype=np.float32)
    for u, (c, e) in enumerate(pairs):
        C[u, :len(c)], E[u, :len(e)] = c, e
    got = pkg["scores"](dev(E), dev(C), 16000, True, lengths)
    assert torch.equal(got, pkg["taal"](C, E, fs=16000, extended=True, lengths=lengths))


# ---- 6. the module ----
def _batch16():
    pairs = [sc.case_pair(lc.case(n)) for n in (7, 11, 6)]
    lengths = [len(e) for _, e in pairs]
    C, E = np.zeros((3, 9600), dtype=np.float32), np.zeros((3, 9600), dtype=np.float32)
    for u, (c, e) in enumerate(pairs):
        C[u, :len(c)], E[u, :len(e)] = c, e
    return C, E, lengths


def test_module_value_gradient_and_config(pkg, monkeypatch):
    C, E, lengths = _batch16()
    for ext in sc.MEASURES:
        s = pkg["scores"](dev(E), dev(C), 16000, ext, lengths).cpu().numpy()
        assert s[1] == 1e-5
        Ed, Cd = dev(E).requires_grad_(True), dev(C).requires_grad_(True)
        loss = pkg["loss"](16000, extended=ext)(Ed, Cd, lengths)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss.detach()) == np.float32(-(s[0] + s[2]) / 2)
        loss.backward()
        assert Cd.grad is None and not Ed.grad[1].any() and Ed.grad[0].any() and Ed.grad[2].any()
        _, g = grad_of(pkg, C, E, 16000, ext, lengths, torch.tensor([-0.5, 0.0, -0.5]).cuda())
        assert np.array_equal(g, Ed.grad.cpu().numpy())
    c, e = sc.case_pair(lc.case(11))                         # no utterance qualifies
    Ed = dev(np.stack([e, e])).requires_grad_(True)
    loss = pkg["loss"](16000)(Ed, dev(np.stack([c, c])))
    loss.backward()
    assert float(loss.detach()) == 0.0 and not Ed.grad.any()
    c, e = sc.case_pair(lc.case(10))                         # extended=None follows config at each call; 1-D input
    m = pkg["loss"]()
    assert m.sample_rate == 8000
    monkeypatch.setattr(pkg["config"], "STOI_EXTENDED", False)
    plain = float(m(dev(e), dev(c)))
    monkeypatch.setattr(pkg["config"], "STOI_EXTENDED", True)
    extended = float(m(dev(e), dev(c)))
    assert plain == float(pkg["loss"](8000, extended=False)(dev(e), dev(c))) != extended
    assert extended == float(pkg["loss"](8000, extended=True)(dev(e), dev(c)))


def test_module_refuses_before_a_launch(pkg, monkeypatch):
    from sincformer_metacog_speech_enhancement_amd import ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a, **k: calls.append(a))
    m = pkg["loss"](16000)
    x = torch.zeros(2, 6000).cuda()
    with pytest.raises(RuntimeError, match="CPU"):
        m(x.cpu(), x)
    with pytest.raises(RuntimeError, match="CPU"):
        m(x, x.cpu())
    with pytest.raises(ValueError, match="one shape"):
        m(x, x[:, :5000])
    with pytest.raises(ValueError, match="one shape"):
        m(x.double(), x.double())
    for bad in ([6000, 6001], [-1, 6000], [6000]):
        with pytest.raises(ValueError, match="lengths"):
            m(x, x, bad)
    with pytest.raises(NotImplementedError):
        pkg["loss"](44100)
    assert not calls


def test_second_call_with_the_same_lengths_does_not_synchronise(pkg):
    C, E, lengths = _batch16()
    Cd = dev(C)
    m = pkg["loss"](16000, extended=True)
    first = dev(E).requires_grad_(True)
    m(first, Cd, lengths).backward()
    second = dev(E).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = m(second, Cd, list(lengths))
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first.grad, second.grad)


# ---- 7. composition ----
def test_gradient_reaches_both_spectrum_planes_through_the_istft(pkg):
    c, _ = sc.case_pair(lc.case(10))                         # 8 kHz, 5000 samples
    L, nf, hop, wn = len(c), 256, 80, 160
    T, F = 1 + L // hop, nf // 2 + 1
    r = torch.Generator().manual_seed(3)
    re = (torch.randn(1, T, F, generator=r) * 0.1).cuda().requires_grad_(True)
    im = (torch.randn(1, T, F, generator=r) * 0.1).cuda().requires_grad_(True)
    wav = pkg["train"].IstftFunction.apply(re, im, L, nf, hop, wn)
    loss = pkg["loss"](8000, extended=True)(wav, dev(c)[None])
    loss.backward()
    for gr in (re.grad, im.grad):
        assert torch.isfinite(gr).all() and float(gr.abs().max()) > 0.0
    assert abs(float(loss.detach())) > 1e-5


@pytest.mark.parametrize("ext", sc.MEASURES)
def test_ten_ascent_steps_raise_the_score(pkg, ext):
    cs = lc.case(lc.ASCENT_CASE)
    c, e = sc.case_pair(cs)
    before = pkg["taal"](c, e, fs=cs[1], extended=ext)
    Cd, x = dev(c), dev(e)
    for _ in range(lc.ASCENT_STEPS):
        x = x.detach().requires_grad_(True)
        pkg["scores"](x, Cd, cs[1], ext).sum().backward()
        x = x + lc.ASCENT_STEP * x.grad
    after = pkg["taal"](c, x.detach().cpu().numpy(), fs=cs[1], extended=ext)
    print("ROW | ascent %s | before %.6f | after %.6f" % ("estoi" if ext else "stoi", before, after))
    assert after - before >= 10.0 * sc.evaluated()[(lc.ASCENT_CASE, ext)]["e32"] and after - before > 1e-2
