"""The gammatone T-F analysis on the device (csrc/gammatone.hip through signal_processing.GammatoneFilterbank and
training.gammatone_mask_target) against the float64 restatement of tests/gammatone_cases.py.

Every row goes through helpers.check_row with k = 16: the device result within 16 x e32 of the float64 restatement, e32 = the
float32 evaluation of the same restatement on the CPU against the float64 one, on the same inputs.
  filter      [C, L] of the FIR bank.
  blocks      the five sums per hop-block (each sum a slice of its own).
  mag         the frame powers: a sum of non-negative terms, held to its own e32 without a sum bound.
  bins        the real and imaginary part of S[cf_bin], each over the Cauchy-Schwarz norm sqrt(w sum f^2) of its frame.
  phase       by angular distance, per unit: with e the bound of the bin row, 2 e / (|S64[cf_bin]| / norm); units where that
              exceeds 0.1 rad are skipped, at most 1 % of a case (tests/test_gammatone_host.py asserts the cap on the CPU).
Silent frames (all samples and all history inside the exact zeros) must be exactly 0 in every plane.  Dead units (below the fp32
tap operand's range, gammatone_cases' docstring) are in the rows measured against the plane and not in bins / phase.
Every row prints `ROW | ...`; profiles/README.md keeps the table."""
import numpy as np
import pytest
import torch

import gammatone_cases as gc
import helpers as hp
import mask_cases as mc

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd import masks, ops, training
    from sincformer_metacog_speech_enhancement_amd.signal_processing import GammatoneFilterbank
    banks = {name: GammatoneFilterbank(**kw) for name, kw in gc.BANKS.items()}
    return {"banks": banks, "ops": ops, "training": training, "masks": masks}


def _run(dev, name, **kw):
    _, bname, _, _, _, (frame, hop, N) = gc.CASES[name]
    out = dev["banks"][bname].get_tf_magnitudes(gc.case_signal(name).cuda(), frame, hop, N, want_bins=True, **kw)
    torch.cuda.synchronize()
    return dict(zip(("mag", "phase", "re", "im"), (o.cpu() for o in out)))


def _check_planes(name, got, tag=""):
    a64, a32 = gc.analysis(name, F64), gc.analysis(name, F32)
    n = a64["norm"]
    assert got["mag"].shape == a64["mag"].shape and got["mag"].dtype == torch.float32
    hp.check_row("mag %s%s" % (name, tag), got["mag"], a64["mag"], a32["sums"]["mag"], gc.K)
    stack = lambda re, im: torch.stack([gc.normalised(re, n), gc.normalised(im, n)])
    hp.check_row("bins %s%s" % (name, tag), stack(got["re"], got["im"]), stack(a64["re"], a64["im"]),
                 stack(a32["sums"]["re"], a32["sums"]["im"]), gc.K)
    bound, keep, skipped = gc.phase_bound(name)
    d = gc.angular_distance(got["phase"], a64["phase"])
    worst = float((d[keep] / bound[keep]).max()) if keep.any() else 0.0
    print("ROW | phase %s%s | largest bound %.2e rad | worst observed / bound %.3f | %d of %d units skipped" % (
        name, tag, float(bound.max()), worst, skipped, keep.numel()))
    assert skipped <= 0.01 * keep.numel() and bool((d[keep] <= bound[keep]).all())
    first, last = gc.silent_frames(name)
    for q in ("mag", "phase", "re", "im"):
        assert bool((got[q][:, first:last] == 0).all()), (name, q, "silent frames are not exactly 0")
    return last - first


@pytest.mark.parametrize("name", list(gc.CASES))
def test_tf_planes(dev, name):
    silent = _check_planes(name, _run(dev, name))
    if name in ("d1041", "d1153", "d2403", "c1153"):
        assert silent == 1


@pytest.mark.parametrize("name", ["d160", "d559", "d1153", "k1153", "c239"])
def test_filter_row(dev, name):
    b = dev["banks"][gc.CASES[name][1]]
    x = gc.case_signal(name).cuda()
    y = b.filter(x).cpu()
    a64, a32 = gc.analysis(name, F64), gc.analysis(name, F32)
    assert y.shape == a64["y"].shape
    hp.check_row("filter " + name, y, a64["y"], a32["y"], gc.K)
    a, z = gc.zero_stretch(x.numel())
    taps = len(b.impulse_responses[0])
    assert bool((y[:, a + taps - 1:a + z] == 0).all())                     # behind the taps' reach inside the zeros: exactly 0
    _, _, _, _, _, (frame, hop, _) = gc.CASES[name]
    f = b.filter_to_frames(x, frame, hop).cpu()
    assert torch.equal(f, y.unfold(-1, frame, hop))                         # data movement only


@pytest.mark.parametrize("name", ["d240", "d1153", "k2403", "c1153"])
def test_block_sums_row(dev, name):
    _, bname, _, _, _, (frame, hop, N) = gc.CASES[name]
    got = dev["banks"][bname].block_sums(gc.case_signal(name).cuda(), hop, N).cpu().permute(1, 0, 2)     # [C, nblocks, 5]
    a64, a32 = gc.analysis(name, F64), gc.analysis(name, F32)
    assert got.shape == a64["blocks"].shape
    names = ("s2", "s1", "sp", "sc", "ss")
    hp.check_row("blocks " + name, got, a64["blocks"], a32["blocks"], gc.K,
                 slices={q: (lambda t, i=i: t[..., i]) for i, q in enumerate(names)})


def _ragged():
    lengths = [gc.CASES[n][2] for n in gc.RAGGED]
    x = torch.zeros(len(lengths), max(lengths))
    for i, n in enumerate(gc.RAGGED):
        x[i, :lengths[i]] = gc.case_signal(n)
    return x, lengths


def test_ragged_batch_rows_equal_the_single_calls_bitwise(dev):
    b = dev["banks"]["default"]
    x, lengths = _ragged()
    batch = [o.cpu() for o in b.get_tf_magnitudes(x.cuda(), want_bins=True, lengths=lengths)]
    again = [o.cpu() for o in b.get_tf_magnitudes(x.cuda(), want_bins=True, lengths=lengths)]
    assert all(torch.equal(p, q) for p, q in zip(batch, again))           # two runs: the same bits
    T = batch[0].shape[2]
    assert T == (max(lengths) - gc.FRAME) // gc.HOP + 1
    for i, name in enumerate(gc.RAGGED):
        alone = _run(dev, name)
        Tb = alone["mag"].shape[1]
        for plane, q in zip(batch, ("mag", "phase", "re", "im")):
            assert torch.equal(plane[i, :, :Tb], alone[q]), (name, q)
            assert bool((plane[i, :, Tb:] == 0).all()), (name, q)
        # the padded plane is the row that the 'last partial block' mutant fails (tests/test_gammatone_host.py)
        a64, a32 = gc.analysis(name, F64), gc.analysis(name, F32)
        hp.check_row("mag padded " + name, batch[0][i], gc.padded(a64["mag"], T), gc.padded(a32["sums"]["mag"], T), gc.K)
    y = b.filter(x.cuda(), lengths=lengths).cpu()
    for i, name in enumerate(gc.RAGGED):
        assert torch.equal(y[i, :, :lengths[i]], b.filter(gc.case_signal(name).cuda()).cpu())
        assert bool((y[i, :, lengths[i]:] == 0).all())


@pytest.mark.parametrize("name", ["d239", "d1153", "d2403", "k2403", "c1153"])
def test_fused_and_unfused_routes_agree(dev, name):
    ops = dev["ops"]
    fused = _run(dev, name)
    ops.set_gammatone_fused(False)
    try:
        unfused = _run(dev, name)
        again = _run(dev, name)
    finally:
        ops.set_gammatone_fused(True)
    assert all(torch.equal(unfused[q], again[q]) for q in unfused)
    _check_planes(name, unfused, " unfused")
    _check_planes(name, fused, " fused")


def test_bad_arguments_are_refused(dev):
    b = dev["banks"]["default"]
    x = gc.case_signal("d240").cuda()
    with pytest.raises(ValueError, match="shorter than one frame"):
        b.get_tf_magnitudes(x[:159])
    with pytest.raises(ValueError, match="even size"):
        b.get_tf_magnitudes(x, fft_size=255)
    with pytest.raises(ValueError, match="lengths"):
        b.get_tf_magnitudes(x.view(1, -1), lengths=[241])
    with pytest.raises(TypeError):
        b.get_tf_magnitudes(x.double())
    m, p = b.get_tf_magnitudes(x)
    assert m.shape == p.shape == (64, 2) and not m.requires_grad


def _target_reference(dtype, names, noise, kind):
    """[T, C] per utterance: the restatement's planes chained with mask_cases' formulas"""
    out = []
    b = gc.bank("default")
    bins = b.cf_bins(gc.FFT)
    h = gc.taps_of(b, dtype)
    for name, nz in zip(names, noise):
        c32 = gc.case_signal(name)
        L = c32.numel()
        n32 = torch.zeros(L)
        n32[:min(L, nz.numel())] = nz[:L]
        c, n, y = c32.to(dtype), n32.to(dtype), (c32 + n32).to(dtype)        # the mix is the caller's: formed in fp32
        planes = []
        for sig in (c, n, y):
            yy = gc.fir(sig, h)
            s = gc.five_sums(gc.frames_of(yy, gc.FRAME, gc.HOP), gc.FFT, bins)
            planes.append(gc.finish(s, gc.FFT))
        cm, nm, ym = (p["mag"] for p in planes)
        cp, npz, yp = (p["phase"] for p in planes)
        if kind == "irm":
            m = mc.irm(cm, nm)
        else:
            rho_s, rho_n = mc.corr(ym, cm, nm)
            m = mc.pcirm(cm, nm, rho_s, rho_n, cp - yp, npz - yp)
        out.append(m.t())
    return out


def test_mask_targets(dev):
    """training.gammatone_mask_target of a ragged batch of two (one noise longer than the utterances, cut; 1-D with a shorter
    noise, zero-padded) for the three mask kinds, at mask_cases' K and absolute bound"""
    names = ("d2403", "d1041")
    lengths = [gc.CASES[n][2] for n in names]
    rng = np.random.RandomState(331)
    noise = torch.from_numpy((0.05 * rng.standard_normal((2, 3000))).astype(np.float32))
    clean = torch.zeros(2, max(lengths))
    for i, n in enumerate(names):
        clean[i, :lengths[i]] = gc.case_signal(n)
    cut = noise[:, :max(lengths)].clone()
    cut[1, lengths[1]:] = 0.0
    noisy = clean + cut
    tgt = dev["training"].gammatone_mask_target
    steps, _ = mc.snr_boundaries()
    got = {k: tgt(clean.cuda(), noise.cuda(), noisy.cuda(), k, lengths=lengths).cpu() for k in ("irm", "pcirm", "opt_pcirm", "other")}
    T = (max(lengths) - gc.FRAME) // gc.HOP + 1
    assert all(g.shape == (2, T, 64) for g in got.values())
    assert torch.equal(got["other"], got["irm"])                         # an unknown mask_type falls back to the IRM
    for kind in ("irm", "pcirm"):
        r64, r32 = _target_reference(F64, names, noise, kind), _target_reference(F32, names, noise, kind)
        for i, name in enumerate(names):
            Tb = r64[i].shape[0]
            bound = mc.check("target %s %s" % (kind, name), got[kind][i, :Tb], r64[i], r32[i])
            if kind == "pcirm":
                near = mc.near_boundary(r64[i], steps, bound)
                share = 1.0 - float(near.double().mean())
                q = mc.quantize(r64[i], steps).float()
                print("ROW | target opt_pcirm %s | %.1f %% of the units compared" % (name, 100.0 * share))
                assert share >= 0.95
                assert torch.equal(got["opt_pcirm"][i, :Tb][~near], q[~near])
    one = tgt(clean[1, :lengths[1]].cuda(), noise[1, :700].cuda(), (clean[1, :lengths[1]] + torch.nn.functional.pad(
        noise[1, :700], (0, lengths[1] - 700))).cuda(), "irm").cpu()
    assert one.shape == ((lengths[1] - gc.FRAME) // gc.HOP + 1, 64) and bool(torch.isfinite(one).all())


def test_planes_feed_the_pso_search(dev):
    """get_tf_magnitudes' planes through compute_pcirm and compute_opt_pcirm(use_pso=True) with a small swarm"""
    m, b = dev["masks"], dev["banks"]["default"]
    clean = gc.case_signal("d2403")
    rng = np.random.RandomState(332)
    noise = torch.from_numpy((0.05 * rng.standard_normal(clean.numel())).astype(np.float32))
    noisy = clean + noise
    mag, ph = b.get_tf_magnitudes(torch.stack([clean, noise, noisy]).cuda())
    rho_s, rho_n = m.compute_correlation_coefficients(mag[2], mag[0], mag[1])
    phi1, phi2 = m.compute_phase_differences(ph[2], ph[0], ph[1])
    pcirm = m.compute_pcirm(mag[0], mag[1], rho_s, rho_n, phi1, phi2)
    mask, steps, middle = m.compute_opt_pcirm(pcirm, noisy.cuda(), clean.cuda(), use_pso=True,
                                              pso_config={"num_particles": 6, "max_iter": 3})
    torch.cuda.synchronize()
    assert mask.shape == pcirm.shape == (64, 29) and bool(torch.isfinite(mask).all()) and 0.0 <= float(middle) <= 1.0
