"""The ragged EnhancementPath on the MI355X: seven utterances of different lengths in one pass, each result what the utterance gets
alone.  The case set and its reasons: tests/ragged_path_cases.py.  Every ragged pass of this file runs on a batch whose samples
beyond each length are NaN and whose intermediate buffers start as NaN (functional._ragged_empty): a read beyond a length, or an
element left unwritten, shows as a NaN or as a difference.

  1. company: masks, sigma and enhanced samples of an utterance are bitwise the same alone, in the batch, in the batch reversed
     and in a batch padded to a longer row - exact, no tolerance.
  2. kernels: every launch of a new entry point inside the ragged pass against its dense entry point inside the dense pass on
     [1, L_b]: outputs and GroupNorm partials / scale / shift bitwise equal on the valid rows, zeros where the contract says
     zeros, the NaN guard rows intact where it says untouched.
  3. the path against the oracle on each utterance alone (CPU), with the bounds test_ragged_gpu.py applies to the packed
     SpeechEnhancer: mask RMSE <= 1e-3 (the project's contract), waveform relative RMSE < 2e-2 (mixed) / 3e-3 (fp16).
  4. the path against the dense call on [1, L_b]: the front end bitwise; masks and waveform bitwise or within the bounds of 3,
     printed per utterance.
  5. enhance_batch == forward_ragged, bit for bit, with the input lengths.
  6. a second call with the same lengths makes no synchronising call up to its download.
  7. the dense path gives the bits it gave before the ragged kernels ran."""
import collections
import contextlib

import numpy as np
import pytest
import torch

import ragged_path_cases as rp
from helpers import rmse, rel_rmse
from oracle import sfm_oracle as orc

pytestmark = pytest.mark.gpu

HARD_BOUND = {"mixed": 1e-3, "fp16": 1e-3}          # tests/test_ragged_gpu.py: HARD_BOUND, WAVE_BOUND (bf16: refused by the ragged path)
WAVE_BOUND = {"mixed": 2e-2, "fp16": 3e-3}
KEYS = ("mask_real", "mask_imag", "sigma", "enhanced")


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops, functional
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp

    class NS:
        pass
    ns = NS()
    ns.ops, ns.Fn, ns.cp = ops, functional, cp
    ns.sds = rp.states()
    path = cp.EnhancementPath(sample_rate=rp.FS)
    path.perception.load_state_dict(ns.sds["pa"])
    path.cpea.load_state_dict(ns.sds["cpea"])
    path.msa.load_state_dict(ns.sds["msa"])
    ns.path = path.cuda().eval()
    ns.sigs = rp.waves()
    return ns


@contextlib.contextmanager
def nan_buffers(Fn):
    """every intermediate buffer of the ragged path starts as NaN"""
    keep = Fn._ragged_empty
    Fn._ragged_empty = lambda *shape, device, dtype: torch.full(shape, float("nan"), device=device, dtype=dtype)
    try:
        yield
    finally:
        Fn._ragged_empty = keep


def ragged(pkg, sigs, Lrow=None, want=("mask", "wave")):
    """forward_ragged on the NaN-padded batch -> per utterance {key: CPU tensor}"""
    wave = torch.from_numpy(rp.padded(sigs, Lrow)).cuda()
    with torch.no_grad(), nan_buffers(pkg.Fn):
        out = pkg.path.forward_ragged(wave, [s.size for s in sigs], want=want)
    seg, plan = out["seg"], out["plan"]
    cuts = {"mask_real": seg.frame_counts.tolist(), "mask_imag": seg.frame_counts.tolist(), "sigma": plan.Tpa.tolist(),
            "enhanced": seg.lengths.tolist()}
    parts = {k: out[k].cpu().split(cuts[k], dim=0) for k in KEYS if k in out}
    return [{k: parts[k][b] for k in parts} for b in range(len(sigs))]


def dense(pkg, w):
    with torch.no_grad():
        out = pkg.path(torch.from_numpy(w[None]).cuda())
    return {"mask_real": out["mask_real"][0].cpu(), "mask_imag": out["mask_imag"][0].cpu(), "sigma": out["sigma"][0].cpu(),
            "enhanced": out["enhanced"][0].cpu()}


@pytest.fixture(scope="module")
def batch(pkg):
    pkg.ops.reset_precision()
    return ragged(pkg, pkg.sigs)


def test_every_element_is_written_and_finite(pkg, batch):
    for b, (got, s) in enumerate(zip(batch, pkg.sigs)):
        T = 1 + s.size // rp.HOP
        assert tuple(got["mask_real"].shape) == (T, 129) and tuple(got["enhanced"].shape) == (s.size,)
        assert tuple(got["sigma"].shape) == (rp.conv_shape_chain(s.size)[4],)
        for k in KEYS:
            assert bool(torch.isfinite(got[k]).all()), (b, k)


# ---------------------------------------------------------------------------
# 1. company
# ---------------------------------------------------------------------------
def test_an_utterance_does_not_depend_on_its_company(pkg, batch):
    sigs = pkg.sigs
    alone = [ragged(pkg, [s])[0] for s in sigs]
    rev = ragged(pkg, sigs[::-1])[::-1]
    wide = ragged(pkg, sigs, Lrow=max(rp.LENGTHS) + 333)
    for b in range(len(sigs)):
        for k in KEYS:
            for name, other in (("alone", alone), ("reversed", rev), ("padded to a longer row", wide)):
                assert torch.equal(batch[b][k], other[b][k]), "utterance %d (L %d) %s: %s differs, max %.3e" % (
                    b, rp.LENGTHS[b], name, k, float((batch[b][k] - other[b][k]).abs().max()))


# ---------------------------------------------------------------------------
# 2. every launch of a new entry point against its dense one
# ---------------------------------------------------------------------------
def _clone(t):
    return None if t is None else t.detach().clone()


@contextlib.contextmanager
def recording(pkg, rec):
    """append the results of the front end's launches (dense and ragged wrappers alike) and the fusion operand to rec[name]"""
    ops, Fn = pkg.ops, pkg.Fn
    keep = {}

    def wrap(mod, name, pick):
        orig = getattr(mod, name)
        keep[(mod, name)] = orig

        def fn(*a, **kw):
            r = orig(*a, **kw)
            got = pick(a, kw, r)
            if got is not None:
                rec[name].append(tuple(_clone(t) for t in got))
            return r
        setattr(mod, name, fn)

    conv = lambda a, kw, r: (a[4], kw.get("gn_partial"), kw.get("out_s"), kw.get("gn_partial_s"))
    wrap(ops, "sinc_fir16", lambda a, kw, r: (a[2], r[0]))
    wrap(ops, "sinc_fir16_varlen", lambda a, kw, r: (a[3], r[0]))
    wrap(ops, "conv16p", conv)
    wrap(ops, "conv16p_varlen", conv)
    wrap(ops, "gn_finalize", lambda a, kw, r: r)
    wrap(ops, "gn_finalize_varlen", lambda a, kw, r: r)
    wrap(ops, "gn_apply", lambda a, kw, r: (a[3],) if kw.get("act", 0) == 1 and kw.get("x2") is None else None)
    wrap(ops, "gn_apply_varlen", lambda a, kw, r: (a[3],))
    wrap(ops, "headpool", lambda a, kw, r: (a[2], a[3]))
    wrap(ops, "headpool_varlen", lambda a, kw, r: (a[2], a[3]))
    wrap(ops, "bilstm_layer_rows16", lambda a, kw, r: (r,))
    wrap(ops, "bilstm_layer_rows16_varlen", lambda a, kw, r: (r,))
    wrap(Fn, "msa_logits", lambda a, kw, r: (a[0],))
    try:
        yield
    finally:
        for (mod, name), orig in keep.items():
            setattr(mod, name, orig)


def _valid_rest(name, b, got, want, rest):
    """got [rows of the longest, ...] of utterance b: the first rows equal `want`, the rest is NaN ("nan"), zero ("zero") or
    anything ("any")"""
    n = want.shape[0]
    assert torch.equal(got[:n], want), "%s, utterance %d: valid rows differ (max %.3e)" % (
        name, b, float((got[:n].float() - want.float()).abs().max()))
    if rest == "nan":
        assert bool(torch.isnan(got[n:]).all()), "%s, utterance %d: rows beyond the length were written" % (name, b)
    elif rest == "zero":
        assert bool((got[n:] == 0).all()), "%s, utterance %d: rows beyond the length are not zero" % (name, b)


def test_each_ragged_launch_equals_its_dense_launch(pkg):
    ops, Fn, sigs = pkg.ops, pkg.Fn, pkg.sigs
    B = len(sigs)
    rr = collections.defaultdict(list)
    with recording(pkg, rr):
        got = ragged(pkg, sigs)
    plan = Fn.ragged_plan(rp.LENGTHS)
    assert len(rr["conv16p_varlen"]) == 8 and len(rr["gn_finalize_varlen"]) == 12 and len(rr["bilstm_layer_rows16_varlen"]) == 2
    assert not rr["conv16p"] and not rr["sinc_fir16"] and not rr["headpool"] and not rr["bilstm_layer_rows16"]
    wf = 2 * 256 + 4 * 64
    for b, s in enumerate(sigs):
        rd = collections.defaultdict(list)
        with recording(pkg, rd):
            want = dense(pkg, s)
        assert len(rd["conv16p"]) == 8 and len(rd["gn_finalize"]) == 12 and not rd["conv16p_varlen"]
        out_r, part_r = rr["sinc_fir16_varlen"][0]
        out_d, part_d = rd["sinc_fir16"][0]
        _valid_rest("sinc_fir16 out", b, out_r[b], out_d[0], "nan")
        _valid_rest("sinc_fir16 gn_partial", b, part_r[b], part_d[0], "zero")
        for i, (r, d) in enumerate(zip(rr["conv16p_varlen"], rd["conv16p"])):
            for j, rest in ((0, "nan"), (1, "zero"), (2, "nan"), (3, "zero")):
                assert (r[j] is None) == (d[j] is None)
                if r[j] is not None:
                    _valid_rest("conv16p launch %d operand %d" % (i, j), b, r[j][b], d[j][0], rest)
        for i, (r, d) in enumerate(zip(rr["gn_finalize_varlen"], rd["gn_finalize"])):
            assert torch.equal(r[0][b], d[0][0]) and torch.equal(r[1][b], d[1][0]), "gn_finalize launch %d, utterance %d" % (i, b)
        _valid_rest("gn_apply (zeros beyond Tpa)", b, rr["gn_apply_varlen"][0][0][b], rd["gn_apply"][0][0][0], "zero")
        _valid_rest("headpool pooled", b, rr["headpool_varlen"][0][0][b], rd["headpool"][0][0][0], "zero")
        _valid_rest("headpool gn_partial", b, rr["headpool_varlen"][0][1][b], rd["headpool"][0][1][0], "zero")
        T = int(plan.T[b])
        for i, (r, d) in enumerate(zip(rr["bilstm_layer_rows16_varlen"], rd["bilstm_layer_rows16"])):
            _valid_rest("bilstm layer %d" % i, b, r[0].view(B, plan.T_max, -1)[b], d[0].view(T, -1), "zero")
        # the hand-over: the packed fusion operand's front-end columns = pooled latents | CPEA outputs of the dense call
        f0, f1 = int(plan.seg.frame_offsets[b]), int(plan.seg.frame_offsets[b + 1])
        fr, fd = rr["msa_logits"][0][0][f0:f1], rd["msa_logits"][0][0]
        assert torch.equal(fr[:, :wf], fd[:, :wf]), "fusion operand (latents | CPEA), utterance %d" % b
        assert bool(torch.isfinite(fr.float()).all())
        assert torch.equal(got[b]["sigma"], want["sigma"]), "sigma, utterance %d" % b


def test_rows_gather_copies_the_valid_rows_only(pkg):
    ops, Fn = pkg.ops, pkg.Fn
    plan = Fn.ragged_plan(rp.LENGTHS)
    tb, st = plan.tables("cuda"), plan.seg.tables("cuda")
    B, T = plan.B, plan.T_max
    g = torch.Generator().manual_seed(5)
    src = torch.randn(B * T, 24, generator=g).half().cuda()
    dst = torch.full((plan.seg.sum_T + 1, 32), float("nan"), dtype=torch.float16, device="cuda")
    ops.rows_gather32(src, dst[:-1], tb["T"].dev, st["frame_off"], B, T, 20, plan.seg.sum_T)
    want = torch.cat([src.view(B, T, 24)[b, :int(plan.T[b]), :20] for b in range(B)])
    assert torch.equal(dst[:-1, :20], want) and bool(torch.isnan(dst[:, 20:]).all()) and bool(torch.isnan(dst[-1]).all())


# ---------------------------------------------------------------------------
# 3. / 4. the path against the oracle and against the dense call
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle(pkg):
    out = []
    for s in pkg.sigs:
        o = orc.enhance_path(pkg.sds, torch.from_numpy(s[None]), rp.FS)
        out.append({"mask": torch.cat([o["mask_real"], o["mask_imag"]], -1)[0], "enhanced": o["enhanced"][0]})
    return out


@pytest.mark.parametrize("prec", ["mixed", "fp16"])
def test_ragged_path_matches_the_oracle_on_every_utterance(pkg, oracle, prec):
    if prec == "fp16":
        pkg.ops.set_compute_dtype("fp16")
    got = ragged(pkg, pkg.sigs)
    bad = []
    for b, (g, r) in enumerate(zip(got, oracle)):
        m = rmse(torch.cat([g["mask_real"], g["mask_imag"]], -1), r["mask"])
        wv = rel_rmse(g["enhanced"], r["enhanced"])
        print("ragged %-5s L %4d | mask RMSE %.3e (bound %.0e) | wave rel RMSE %.3e (bound %.0e)" % (
            prec, rp.LENGTHS[b], m, HARD_BOUND[prec], wv, WAVE_BOUND[prec]))
        if not (m <= HARD_BOUND[prec] and wv < WAVE_BOUND[prec]):
            bad.append((b, m, wv))
    assert not bad, bad


def test_ragged_path_against_the_dense_call(pkg, batch):
    bad = []
    for b, s in enumerate(pkg.sigs):
        want = dense(pkg, s)
        assert torch.equal(batch[b]["sigma"], want["sigma"])                 # the front end is bitwise (the rest of it: test 2)
        same = all(torch.equal(batch[b][k], want[k]) for k in ("mask_real", "mask_imag", "enhanced"))
        m = rmse(torch.cat([batch[b]["mask_real"], batch[b]["mask_imag"]], -1), torch.cat([want["mask_real"], want["mask_imag"]], -1))
        wv = rel_rmse(batch[b]["enhanced"], want["enhanced"])
        print("ragged vs dense L %4d: %s | mask RMSE %.3e | wave rel RMSE %.3e" % (
            rp.LENGTHS[b], "bitwise" if same else "other route in the back half", m, wv))
        if not same and not (m <= HARD_BOUND["mixed"] and wv < WAVE_BOUND["mixed"]):
            bad.append((b, m, wv))
    assert not bad, bad


# ---------------------------------------------------------------------------
# 5. - 7.
# ---------------------------------------------------------------------------
def test_enhance_batch_is_the_same_pass(pkg, batch):
    waves = pkg.path.enhance_batch(pkg.sigs)
    assert [w.shape for w in waves] == [(n,) for n in rp.LENGTHS] and all(w.dtype == np.float32 for w in waves)
    for b, w in enumerate(waves):
        assert np.array_equal(w, batch[b]["enhanced"].numpy()), b
    tens = pkg.path.enhance_batch([torch.from_numpy(s) for s in pkg.sigs[:3]])
    assert all(np.array_equal(t, batch[b]["enhanced"].numpy()) for b, t in enumerate(tens))
    assert pkg.path.enhance_batch([]) == []


def test_a_repeated_set_of_lengths_does_not_synchronise(pkg, batch):
    wave = torch.from_numpy(rp.padded(pkg.sigs, fill=0.0)).cuda()
    with torch.no_grad():
        first = pkg.path.forward_ragged(wave, rp.LENGTHS)["enhanced"].clone()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = pkg.path.forward_ragged(wave, rp.LENGTHS)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out["enhanced"], first)
    assert torch.equal(first.cpu(), torch.cat([g["enhanced"] for g in batch]))


def test_the_dense_path_is_unchanged_by_the_ragged_kernels(pkg):
    Fn, path = pkg.Fn, pkg.path
    L = 2049
    noisy = torch.from_numpy(np.stack([s[:L] for s in rp.waves([L + 7, L, L + 500], seed=83)])).cuda()
    pk = path.perception._packed(lambda sd: Fn.pack_perception(sd, path.sample_rate))
    with torch.no_grad():
        before = {k: v.clone() for k, v in path(noisy).items() if isinstance(v, torch.Tensor)}
        (rz, sz, hz), sg = Fn.perception_forward(noisy, pk, latents=False, pool_to=1 + L // rp.HOP, lengths=None)
        front = [t.clone() for t in (rz, sz, hz, sg)]
        path.forward_ragged(noisy, [L, L - 9, L - 400])                      # the ragged kernels run in between
        after = path(noisy)
        (rz, sz, hz), sg = Fn.perception_forward(noisy, pk, latents=False, pool_to=1 + L // rp.HOP, lengths=None)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert all(torch.equal(a, b) for a, b in zip(front, (rz, sz, hz, sg)))
    # ... and on equal lengths the ragged front end is the dense one, bit for bit
    with torch.no_grad(), nan_buffers(Fn):
        (rz2, sz2, hz2), sg2 = Fn.perception_forward(noisy, pk, latents=False, lengths=[L, L, L])
    assert all(torch.equal(a, b) for a, b in zip(front, (rz2, sz2, hz2, sg2)))
