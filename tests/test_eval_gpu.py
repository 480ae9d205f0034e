"""Packed evaluation on the MI355X: a ragged test set scored on the device (SSNR, the STOI fallback, the PESQ fallback).

  1. kernels: every packed (_varlen) entry point against its dense twin run on every utterance ALONE - spectra bitwise, fp64
     accumulators within 1e-9 - on a set with leading, inner and trailing utterances that own no frame.
  2. measures: compute_metrics_packed against the reference's values (tests/golden/g14_eval.npz) with the bounds of
     test_metrics_gpu.py for SSNR / STOI and K_TRANS x e32 for PESQ (e32: the float32-DFT error of the restatement, from
     eval_cases, never from a kernel); any company (the set, its reverse, a subset) within 1e-9; dense compute_pesq.
  3. driver: ConformerPipeline.evaluate_batch - signals bitwise enhance_batch's, scores equal to compute_metrics_packed on
     them and within the bounds of the dense per-utterance calls, 3 passes within 1e-9.
tests/test_eval_host.py shows on the CPU that these bounds separate plausible wrong packed kernels."""
import numpy as np
import pytest
import torch

import eval_cases as ec
import ragged_cases as rc
from helpers import gold, K_TRANS

pytestmark = pytest.mark.gpu

SETS = {"the set": list(range(12)), "reversed": list(range(11, -1, -1)), "a subset": [4, 9, 2, 11, 0, 8, 7]}


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops, functional, evaluation
    from sincformer_metacog_speech_enhancement_amd.evaluation import packed, stoi
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp

    class NS:
        pass
    ns = NS()
    ns.ops, ns.Fn, ns.ev, ns.pk, ns.stoi, ns.cp = ops, functional, evaluation, packed, stoi, cp
    return ns


@pytest.fixture(scope="module")
def case():
    c, x, e = ec.signals()
    return c, x, e


@pytest.fixture(scope="module")
def pesq_bound():
    return K_TRANS * ec.pesq_e32()


def pack(pkg, sigs):
    L = np.asarray([s.size for s in sigs], dtype=np.int64)
    seg = pkg.Fn.PackedSegments(1 + L // 80, L)
    return seg, torch.from_numpy(np.concatenate(sigs)).cuda()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# 1. kernels: packed against dense, per utterance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_ssnr_frames_varlen_against_the_dense_twin(pkg, case, name):
    c, x, e = case
    idx = SETS[name]
    cs, es = [c[i] for i in idx], [e[i] for i in idx]
    seg, cp_ = pack(pkg, cs)
    _, ep_ = pack(pkg, es)
    frame, hop = ec.FRAMINGS["ssnr"]
    tab = seg.metric_tables("cuda", ((frame, hop),))[(frame, hop)]
    acc = pkg.ops.ssnr_frames_varlen(cp_, ep_, seg.tables("cuda")["samp_off"], tab["frame_off"], seg.B, tab["sum"], frame, hop).cpu()
    L = pkg.ops._lib.load()
    for k, (a, b) in enumerate(zip(cs, es)):
        one = torch.zeros(1, 2, device="cuda", dtype=torch.float64)
        da, db = dev(a), dev(b)
        pkg.ops._call("metrics", L.sfm_ssnr_frames, (pkg.ops._p(da), pkg.ops._p(db), pkg.ops._p(one), 1, a.size, frame, hop, 35.0, -10.0,
                                                     pkg.ops._stream()))
        d = float((acc[k] - one.cpu()[0]).abs().max())
        print("ssnr acc | %s | utterance %d (L %d, %d frames) | packed {%.6f, %d} | |packed - dense| %.1e" % (
            name, idx[k], a.size, tab["n"][k], acc[k, 0], acc[k, 1], d))
        assert d <= ec.ACC_BOUND and float(acc[k, 1]) <= tab["n"][k], (name, k)


@pytest.mark.parametrize("measure", ["stoi", "pesq"])
@pytest.mark.parametrize("name", list(SETS))
def test_spectra_and_frame_sums_varlen_against_the_dense_twins(pkg, case, name, measure):
    """the packed DFT rows are bitwise the dense rows (one GEMM row from that row's samples alone); the fp64 frame sums and the
    wave moments agree within 1e-9"""
    c, x, e = case
    idx = SETS[name]
    cs, es = [c[i] for i in idx], [e[i] for i in idx]
    seg, cp_ = pack(pkg, cs)
    _, ep_ = pack(pkg, es)
    frame, hop = ec.FRAMINGS[measure]
    F = frame // 2 + 1
    tab = seg.metric_tables("cuda", ((frame, hop),))[(frame, hop)]
    samp_off = seg.tables("cuda")["samp_off"]
    W = pkg.stoi._dft_operand(frame, torch.device("cuda"), "hann" if measure == "stoi" else "rect")
    pc = pkg.pk._spectra(cp_, W, samp_off, tab, seg.B, frame, hop)
    pe = pkg.pk._spectra(ep_, W, samp_off, tab, seg.B, frame, hop)
    S = pkg.ops.wave_moments_varlen(ep_, cp_, samp_off, seg.B, int(seg.lengths.max()))
    Ls = torch.from_numpy(seg.lengths).cuda().double()
    sc = (1.0 / (torch.sqrt(S[:, 3] / Ls) + 1e-10)).contiguous()
    se = (1.0 / (torch.sqrt(S[:, 2] / Ls) + 1e-10)).contiguous()
    if measure == "stoi":
        acc = pkg.ops.stoi_frames_varlen(pc[0], pc[1], pe[0], pe[1], sc, se, tab["frame_off"], seg.B).cpu()
    else:
        acc = pkg.ops.lsd_frames_varlen(pc[0], pc[1], pe[0], pe[1], tab["frame_off"], seg.B).cpu()
    L = pkg.ops._lib.load()
    off = np.concatenate([[0], np.cumsum(tab["n"])])
    for k, (a, b) in enumerate(zip(cs, es)):
        n = int(tab["n"][k])
        da, db = dev(a).unsqueeze(0), dev(b).unsqueeze(0)
        Sd = torch.zeros(1, 5, device="cuda", dtype=torch.float64)
        pkg.ops._call("loss_reduce", L.sfm_wave_moments, (pkg.ops._p(db), pkg.ops._p(da), pkg.ops._p(Sd), 1, a.size, None, pkg.ops._stream()))
        dm = float((S[k].cpu() - Sd.cpu()[0]).abs().max())
        assert dm <= ec.ACC_BOUND, (name, k, dm)
        if n == 0:
            assert float(acc[k]) == 0.0
            print("%s | %s | utterance %d (L %d) owns no frame | moments |packed - dense| %.1e" % (measure, name, idx[k], a.size, dm))
            continue
        dense = []
        for sig in (da, db):
            re = torch.empty(1, n, F, device="cuda", dtype=torch.float32)
            im = torch.empty(1, n, F, device="cuda", dtype=torch.float32)
            pkg.ops.framed_gemm(sig, W, re, B=1, M=n, Ls=a.size, sig_batch_stride=a.size, hop=hop, padl=0, K=frame, N=2 * F,
                                o_batch_stride=n * F, ldm=F, ldn=1, mode=0, out2=im, nsplit=F)
            dense += [re, im]
        for part, p, d in zip(("clean re", "clean im", "enh re", "enh im"), pc + pe, dense):
            assert torch.equal(p[off[k]:off[k + 1]], d[0]), (name, k, part)
        if measure == "stoi":
            one = torch.zeros(1, device="cuda", dtype=torch.float64)
            sck, sek = sc[k:k + 1].clone(), se[k:k + 1].clone()
            pkg.ops._call("metrics", L.sfm_stoi_frames, tuple(pkg.ops._p(t) for t in dense) + (
                pkg.ops._p(sck), pkg.ops._p(sek), pkg.ops._p(one), 1, n, F, pkg.ops._stream()))
        else:
            one = pkg.ops.lsd_frames(*dense)
        d = abs(float(acc[k]) - float(one.cpu()[0]))
        print("%s | %s | utterance %d (L %d, %d frames) | spectra bitwise | sum %.9f |packed - dense| %.1e | moments %.1e" % (
            measure, name, idx[k], a.size, n, acc[k], d, dm))
        assert d <= ec.ACC_BOUND, (name, k, d)


# ---------------------------------------------------------------------------
# 1b. the long pack: every wave walks several consecutive frames, across utterances and over the ones that own no frame
# (on the 12-utterance set a wave owns ONE frame and never flushes inside its run: eval_cases.LONG_ORDER, test_eval_host.py)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_pack(pkg, case):
    c, x, e = case
    seg, cp_ = pack(pkg, [c[i] for i in ec.LONG_ORDER])
    _, ep_ = pack(pkg, [e[i] for i in ec.LONG_ORDER])
    return seg, cp_, ep_, torch.tensor(ec.LONG_ORDER)


def test_long_pack_ssnr_frames_varlen_against_the_dense_twin(pkg, case, long_pack):
    c, x, e = case
    seg, cp_, ep_, order = long_pack
    frame, hop = ec.FRAMINGS["ssnr"]
    tab = seg.metric_tables("cuda", ((frame, hop),))[(frame, hop)]
    per = ec.run_length(tab["sum"])
    assert per == 17 and tab["n"][0] == 0 and tab["n"][-1] == 0
    acc = pkg.ops.ssnr_frames_varlen(cp_, ep_, seg.tables("cuda")["samp_off"], tab["frame_off"], seg.B, tab["sum"], frame, hop).cpu()
    L = pkg.ops._lib.load()
    dense = torch.zeros(12, 2, dtype=torch.float64)
    for i, (a, b) in enumerate(zip(c, e)):
        one = torch.zeros(1, 2, device="cuda", dtype=torch.float64)
        da, db = dev(a), dev(b)
        pkg.ops._call("metrics", L.sfm_ssnr_frames, (pkg.ops._p(da), pkg.ops._p(db), pkg.ops._p(one), 1, a.size, frame, hop, 35.0, -10.0,
                                                     pkg.ops._stream()))
        dense[i] = one.cpu()[0]
    d = (acc - dense[order]).abs().amax(dim=1)
    print("long pack | ssnr | %d utterances, %d frames, %d per wave | max |packed - dense| %.1e (utterance %d of the pack)" % (
        seg.B, tab["sum"], per, float(d.max()), int(d.argmax())))
    assert float(d.max()) <= ec.ACC_BOUND
    assert torch.equal(acc[:, 1], dense[order][:, 1])                       # the counts of kept frames, exactly


@pytest.mark.parametrize("measure", ["stoi", "pesq"])
def test_long_pack_spectra_and_frame_sums_varlen_against_the_dense_twins(pkg, case, long_pack, measure):
    c, x, e = case
    seg, cp_, ep_, order = long_pack
    frame, hop = ec.FRAMINGS[measure]
    F = frame // 2 + 1
    tab = seg.metric_tables("cuda", ((frame, hop),))[(frame, hop)]
    per = ec.run_length(tab["sum"])
    assert per == {"stoi": 7, "pesq": 5}[measure] and tab["n"][0] == 0 and tab["n"][-1] == 0
    samp_off = seg.tables("cuda")["samp_off"]
    W = pkg.stoi._dft_operand(frame, torch.device("cuda"), "hann" if measure == "stoi" else "rect")
    pc = pkg.pk._spectra(cp_, W, samp_off, tab, seg.B, frame, hop)
    pe = pkg.pk._spectra(ep_, W, samp_off, tab, seg.B, frame, hop)
    S = pkg.ops.wave_moments_varlen(ep_, cp_, samp_off, seg.B, int(seg.lengths.max()))
    Ls = torch.from_numpy(seg.lengths).cuda().double()
    sc = (1.0 / (torch.sqrt(S[:, 3] / Ls) + 1e-10)).contiguous()
    se = (1.0 / (torch.sqrt(S[:, 2] / Ls) + 1e-10)).contiguous()
    if measure == "stoi":
        acc = pkg.ops.stoi_frames_varlen(pc[0], pc[1], pe[0], pe[1], sc, se, tab["frame_off"], seg.B).cpu()
    else:
        acc = pkg.ops.lsd_frames_varlen(pc[0], pc[1], pe[0], pe[1], tab["frame_off"], seg.B).cpu()
    # the dense twins, once per distinct utterance (the first copy's rms factors: every copy has the same samples)
    L = pkg.ops._lib.load()
    first = {i: ec.LONG_ORDER.index(i) for i in range(12)}
    dense_spec, dense_sum, dense_mom = {}, torch.zeros(12, dtype=torch.float64), torch.zeros(12, 5, dtype=torch.float64)
    for i, (a, b) in enumerate(zip(c, e)):
        n = ec.frame_count(a.size, frame, hop)
        da, db = dev(a).unsqueeze(0), dev(b).unsqueeze(0)
        Sd = torch.zeros(1, 5, device="cuda", dtype=torch.float64)
        pkg.ops._call("loss_reduce", L.sfm_wave_moments, (pkg.ops._p(db), pkg.ops._p(da), pkg.ops._p(Sd), 1, a.size, None, pkg.ops._stream()))
        dense_mom[i] = Sd.cpu()[0]
        parts = []
        for sig in (da, db):
            re = torch.empty(1, max(n, 1), F, device="cuda", dtype=torch.float32)
            im = torch.empty(1, max(n, 1), F, device="cuda", dtype=torch.float32)
            if n:
                pkg.ops.framed_gemm(sig, W, re, B=1, M=n, Ls=a.size, sig_batch_stride=a.size, hop=hop, padl=0, K=frame, N=2 * F,
                                    o_batch_stride=n * F, ldm=F, ldn=1, mode=0, out2=im, nsplit=F)
            parts += [re[:, :n], im[:, :n]]
        dense_spec[i] = parts
        if n and measure == "stoi":
            one = torch.zeros(1, device="cuda", dtype=torch.float64)
            k = first[i]
            sck, sek = sc[k:k + 1].clone(), se[k:k + 1].clone()
            full = [t.contiguous() for t in parts]
            pkg.ops._call("metrics", L.sfm_stoi_frames, tuple(pkg.ops._p(t) for t in full) + (
                pkg.ops._p(sck), pkg.ops._p(sek), pkg.ops._p(one), 1, n, F, pkg.ops._stream()))
            dense_sum[i] = one.cpu()[0]
        elif n:
            dense_sum[i] = pkg.ops.lsd_frames(*[t.contiguous() for t in parts]).cpu()[0]
    for j, (part, p) in enumerate(zip(("clean re", "clean im", "enh re", "enh im"), pc + pe)):
        want = torch.cat([dense_spec[i][j][0] for i in ec.LONG_ORDER])
        assert torch.equal(p, want), part                                      # bitwise, every row of the pack
    dm = float((S.cpu() - dense_mom[order]).abs().max())
    d = (acc - dense_sum[order]).abs()
    print("long pack | %s | %d utterances, %d frames, %d per wave | spectra bitwise | max |packed - dense| sums %.1e (utterance %d of "
          "the pack), moments %.1e" % (measure, seg.B, tab["sum"], per, float(d.max()), int(d.argmax()), dm))
    assert float(d.max()) <= ec.ACC_BOUND and dm <= ec.ACC_BOUND
    assert all(float(acc[k]) == 0.0 for k in np.nonzero(tab["n"] == 0)[0][:50])


def test_long_pack_measures_equal_the_short_pack_and_the_reference(pkg, case, long_pack, pesq_bound):
    c, x, e = case
    seg, cp_, ep_, order = long_pack
    g = gold("g14_eval")
    small = pkg.ev.compute_metrics_packed(c, e, fs=ec.FS)
    got = pkg.ev.compute_metrics_packed(cp_, ep_, seg, ec.FS)
    bounds = {"ssnr": ec.SSNR_BOUND, "stoi": ec.STOI_BOUND, "pesq": pesq_bound}
    for m in ec.METRICS:
        v = got[m].cpu()
        d_small = float((v - small[m].cpu()[order]).abs().max())
        d_ref = float((v - torch.from_numpy(g[m])[order]).abs().max())
        print("long pack | %s | max |long - 12-utterance pack| %.1e | max |long - reference| %.2e (bound %.1e)" % (m, d_small, d_ref, bounds[m]))
        assert d_small <= ec.ACC_BOUND and d_ref <= bounds[m], (m, d_small, d_ref)


# ---------------------------------------------------------------------------
# 2. the measures
# ---------------------------------------------------------------------------
def test_packed_measures_against_the_reference_values(pkg, case, pesq_bound):
    c, x, e = case
    g = gold("g14_eval")
    seg, cp_ = pack(pkg, c)
    _, ep_ = pack(pkg, e)
    got = pkg.ev.compute_metrics_packed(cp_, ep_, seg, ec.FS)
    assert sorted(got) == sorted(ec.METRICS) and all(v.is_cuda and v.dtype == torch.float64 and v.shape == (12,) for v in got.values())
    bounds = {"ssnr": ec.SSNR_BOUND, "stoi": ec.STOI_BOUND, "pesq": pesq_bound}
    bad = []
    for m in ec.METRICS:
        v = got[m].cpu().numpy()
        for i, L in enumerate(ec.LENGTHS):
            d = abs(v[i] - g[m][i])
            print("PARITY | %s | utterance %2d (L %5d) | GPU %.9f | reference %.9f | |err| %.2e | bound %.2e" % (
                m, i, L, v[i], g[m][i], d, bounds[m]))
            if not d <= bounds[m]:
                bad.append((m, i, d))
    assert not bad, bad
    # the edge semantics, exactly
    at = ec.LENGTHS.index
    s, t, p = (got[m].cpu().numpy() for m in ("ssnr", "stoi", "pesq"))
    assert s[at(159)] == 0.0 and s[at(129)] == 0.0 and t[at(400)] == 0.0 and t[at(129)] == 0.0 and p[at(511)] == 1.0 and p[at(129)] == 1.0


def test_identical_pair_and_a_pack_that_owns_no_frame(pkg, pesq_bound):
    ic, ie = ec.identical_pair()
    g = gold("g14_eval")["identical"]
    got = pkg.ev.compute_metrics_packed([ic], [ie], fs=ec.FS)
    v = [float(got[m][0]) for m in ("ssnr", "stoi", "pesq")]
    print("PARITY | identical pair | GPU ssnr %.9f stoi %.9f pesq %.9f | reference %s" % (v[0], v[1], v[2], g.tolist()))
    assert abs(v[0] - g[0]) <= ec.SSNR_BOUND and abs(v[1] - g[1]) <= ec.STOI_BOUND and abs(v[2] - g[2]) <= pesq_bound
    c, _, e = ec.signals()
    none = pkg.ev.compute_metrics_packed([c[4], c[11][:150]], [e[4], e[11]], fs=ec.FS)          # 129 and 150 samples
    assert none["ssnr"].tolist() == [0.0, 0.0] and none["stoi"].tolist() == [0.0, 0.0] and none["pesq"].tolist() == [1.0, 1.0]
    only = pkg.ev.compute_metrics_packed([c[0]], [e[0]], fs=ec.FS, metrics=("ssnr",))
    assert list(only) == ["ssnr"]
    with pytest.raises(ValueError):
        pkg.ev.compute_metrics_packed([c[0]], [e[0]], fs=ec.FS, metrics=("csii",))
    assert pkg.ev.compute_metrics_packed([], [], fs=ec.FS)["pesq"].shape == (0,)


def test_an_utterance_gets_the_same_scores_in_any_company(pkg, case):
    c, x, e = case
    res = {}
    for name, idx in SETS.items():
        got = pkg.ev.compute_metrics_packed([c[i] for i in idx], [e[i] for i in idx], fs=ec.FS)
        res[name] = {m: dict(zip(idx, got[m].cpu().numpy())) for m in ec.METRICS}
    for name in ("reversed", "a subset"):
        for m in ec.METRICS:
            d = max(abs(res[name][m][i] - res["the set"][m][i]) for i in SETS[name])
            print("company | %s | %s | max |difference to the set| %.1e" % (name, m, d))
            assert d <= ec.ACC_BOUND, (name, m, d)


def test_the_list_form_cuts_every_pair_to_its_shorter_member(pkg, case):
    c, x, e = case
    longer = [np.concatenate([a, np.full(300, 0.05, np.float32)]) for a in e]
    a = pkg.ev.compute_metrics_packed(c, e, fs=ec.FS)
    b = pkg.ev.compute_metrics_packed([torch.from_numpy(s) for s in c], longer, fs=ec.FS)
    for m in ec.METRICS:                                     # (fp64 atomics: the order of a sum differs from run to run)
        assert float((a[m] - b[m]).abs().max()) <= ec.ACC_BOUND, m


def test_dense_compute_pesq_against_the_restatement(pkg, case, pesq_bound):
    c, x, e = case
    for i, (a, b) in enumerate(zip(c, e)):
        got, want = pkg.ev.compute_pesq(a, b, ec.FS), ec.pesq_simplified64(a, b, ec.FS)
        print("compute_pesq 1-D | utterance %2d (L %5d) | GPU %.9f | restatement %.9f | |err| %.2e" % (i, a.size, got, want, abs(got - want)))
        assert isinstance(got, float) and abs(got - want) <= pesq_bound, i
    assert pkg.ev.compute_pesq(c[0], e[0][:300], ec.FS) == 1.0                  # trimmed to the shorter: no frame
    rows = [9, 6, 5, 3]
    n = 3000
    cb, eb = np.stack([c[i][:n] for i in rows]), np.stack([e[i][:n] for i in rows])
    got = pkg.ev.compute_pesq(dev(cb), dev(eb), ec.FS)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (4,)
    for k in range(4):
        want = ec.pesq_simplified64(cb[k], eb[k], ec.FS)
        assert abs(float(got[k]) - want) <= pesq_bound, (k, float(got[k]), want)
    short = pkg.ev.compute_pesq(dev(cb[:, :500]), dev(eb[:, :500]), ec.FS)
    assert short.tolist() == [1.0] * 4
    # 8 kHz: 256-sample frames
    got8, want8 = pkg.ev.compute_pesq(c[9][:5000], e[9][:5000], 8000), ec.pesq_simplified64(c[9][:5000], e[9][:5000], 8000)
    assert abs(got8 - want8) <= pesq_bound


# ---------------------------------------------------------------------------
# 3. the driver
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(pkg):
    p = pkg.cp.ConformerPipeline()
    p.model = pkg.cp.SpeechEnhancer(n_freq=129)
    p.model.load_state_dict(rc.enhancer_state(), strict=True)
    p.model = p.model.cuda().eval()
    return p


def test_evaluate_batch_signals_scores_and_passes(pkg, case, pipe, pesq_bound):
    c, x, e = case
    bounds = {"ssnr": ec.SSNR_BOUND, "stoi": ec.STOI_BOUND, "pesq": pesq_bound}
    waves = pipe.enhance_batch(x)
    res = pipe.evaluate_batch(c, x, fs=ec.FS, return_enhanced=True)
    assert sorted(res) == ["enhanced", "noisy", "signals"]
    assert len(res["signals"]) == 12 and all(np.array_equal(a, b) for a, b in zip(res["signals"], waves))     # bitwise
    for side in ("noisy", "enhanced"):
        assert list(res[side]) == ["stoi", "pesq", "ssnr"]
        assert all(v.dtype == np.float64 and v.shape == (12,) for v in res[side].values())
    # the scores are compute_metrics_packed on those signals ...
    for side, sigs in (("noisy", x), ("enhanced", waves)):
        direct = pkg.ev.compute_metrics_packed(c, sigs, fs=ec.FS)
        for m in ec.METRICS:
            d = float(np.abs(direct[m].cpu().numpy() - res[side][m]).max())
            assert d <= ec.ACC_BOUND, (side, m, d)
    # ... and, within the bounds, the dense per-utterance calls (the oracle on the noisy side)
    ref = ec.scores64(c, x)
    for m in ec.METRICS:
        d = float(np.abs(ref[m] - res["noisy"][m]).max())
        print("evaluate_batch | noisy | %s | max |GPU - oracle| %.2e (bound %.1e)" % (m, d, bounds[m]))
        assert d <= bounds[m], (m, d)
    dense = {"ssnr": pkg.ev.compute_ssnr, "stoi": pkg.ev.compute_stoi, "pesq": pkg.ev.compute_pesq}
    for m in ec.METRICS:
        per = np.array([dense[m](a, w, ec.FS) for a, w in zip(c, waves)])
        d = float(np.abs(per - res["enhanced"][m]).max())
        print("evaluate_batch | enhanced | %s | max |packed - dense per utterance| %.2e (bound %.1e)" % (m, d, bounds[m]))
        assert d <= bounds[m], (m, d)
    # without return_enhanced: the same scores, no signals; a subset of the measures
    plain = pipe.evaluate_batch(c, x, fs=ec.FS)
    assert sorted(plain) == ["enhanced", "noisy"]
    two = pipe.evaluate_batch(c, x, fs=ec.FS, metrics=("ssnr", "stoi"))
    assert list(two["enhanced"]) == ["ssnr", "stoi"]
    for side in ("noisy", "enhanced"):
        for m in ec.METRICS:
            assert float(np.abs(plain[side][m] - res[side][m]).max()) <= ec.ACC_BOUND
        for m in ("ssnr", "stoi"):
            assert float(np.abs(two[side][m] - res[side][m]).max()) <= ec.ACC_BOUND


def test_evaluate_batch_in_three_passes(pkg, case, pipe):
    """max_frames that cuts the list into 3 passes: the same scores within 1e-9, and every pass's scores are
    compute_metrics_packed of the signals it returns"""
    c, x, e = case
    budget = sum(1 + L // 80 for L in ec.LENGTHS) // 2
    assert len(pkg.pk.plan_evaluation(c, x, max_frames=budget)[2]) == 3
    one = pipe.evaluate_batch(c, x, fs=ec.FS, return_enhanced=True)
    split = pipe.evaluate_batch(c, x, fs=ec.FS, max_frames=budget, return_enhanced=True)
    wave = max(float(np.abs(a - b).max()) for a, b in zip(one["signals"], split["signals"]))
    print("three passes | enhanced samples | max |one pass - three passes| %.2e" % wave)
    # every pass here has fewer than 4096 rows, so every GEMM of the model takes the same kernel as in the one-pass run, and a
    # row-wise kernel computes a row from that row alone: the enhanced samples are bitwise the same ("Packed batches")
    assert all(np.array_equal(a, b) for a, b in zip(one["signals"], split["signals"]))
    direct = pkg.ev.compute_metrics_packed(c, split["signals"], fs=ec.FS)
    worst = {}
    for side in ("noisy", "enhanced"):
        for m in ec.METRICS:
            worst[side, m] = float(np.abs(one[side][m] - split[side][m]).max())
            print("three passes | %s | %s | max |difference to the one-pass run| %.2e" % (side, m, worst[side, m]))
    for m in ec.METRICS:
        d = float(np.abs(direct[m].cpu().numpy() - split["enhanced"][m]).max())
        assert d <= ec.ACC_BOUND, (m, d)
    assert all(v <= ec.ACC_BOUND for v in worst.values()), worst


def test_evaluate_batch_edges(pkg, case, pipe):
    c, x, e = case
    empty = pipe.evaluate_batch([], [], return_enhanced=True)
    assert empty["signals"] == [] and all(v.shape == (0,) and v.dtype == np.float64 for s in ("noisy", "enhanced") for v in empty[s].values())
    with pytest.raises(ValueError, match=r"signal 1 .*L=100"):
        pipe.evaluate_batch([c[0], c[1]], [x[0], x[1][:100]])
    with pytest.raises(ValueError):
        pipe.evaluate_batch([c[0]], [x[0]], metrics=("nope",))
    # pairs of unequal lengths are cut to the shorter member before anything else
    a = pipe.evaluate_batch([c[0], c[5][:3000]], [x[0][:1500], x[5]], fs=ec.FS, return_enhanced=True)
    assert [s.size for s in a["signals"]] == [1500, 3000]
    b = pipe.evaluate_batch([c[0][:1500], c[5][:3000]], [x[0][:1500], x[5][:3000]], fs=ec.FS)
    for m in ec.METRICS:
        assert float(np.abs(a["enhanced"][m] - b["enhanced"][m]).max()) <= ec.ACC_BOUND, m
