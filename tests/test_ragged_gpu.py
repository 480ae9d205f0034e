"""Packed (variable-length) inference on the MI355X: utterances of different lengths enhanced in one pass, each result equal to
what that utterance gets alone.

  1. path vs the oracle run on every utterance ALONE, per utterance and per precision, with the bounds the dense path is
     held to (test_modules_gpu.HARD_BOUND, the waveform bounds of test_speech_enhancer_vs_golden, helpers.WIDTH_EVAL_TOL at
     the reference's small test size).  The dense one-signal path meets those bounds on every utterance of the set, T = 2
     included (tools/ragged_parity.py -> profiles/r05/ragged_parity.txt), so the packed path is held to them everywhere.
  2. independence of the company: the same signals in another order give bitwise the same result per signal.
  3. the five new entry points against a float64 evaluation per utterance of the same 16-bit-rounded inputs, with the
     generators, scales and max |err| tolerances of the dense twins in test_kernels_gpu.py.
  4. forward_packed refuses training mode; nothing in a pass loops over utterances on the host.
tests/test_ragged_host.py shows on the CPU that the bounds used here separate plausible wrong packed forwards."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ragged_cases as rc
from helpers import arr, maxerr, rmse, rel_rmse, frame64, dft64, istft64, WIDTH_EVAL_TOL
from oracle import sfm_oracle as orc

pytestmark = pytest.mark.gpu

PRECISIONS = ["mixed", "fp16", "bf16"]
HARD_BOUND = {"mixed": 1e-3, "fp16": 1e-3, "bf16": 2e-3}        # test_modules_gpu.HARD_BOUND
WAVE_BOUND = {"mixed": 2e-2, "fp16": 3e-3, "bf16": 2e-2}        # test_speech_enhancer_vs_golden
DTYPES = [torch.bfloat16, torch.float16]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}    # test_kernels_gpu.EPS

# frame counts of the kernel tests: T = 1 and 2, a multiple of the 128-row query tile (and of the 64-frame convolution tile),
# tile + 1, one utterance of 1100 frames next to 1-frame ones
MIXED_T = [1, 2, 128, 129, 1, 1100, 1, 64, 65, 200]
ONE_T = [300]


def many_T():
    """300 utterances of 100..700 frames: 4 heads x 1 120 query tiles, far more work items than CUs"""
    return np.random.RandomState(17).randint(100, 701, 300).tolist()


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops, functional
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp

    class NS:
        pass
    ns = NS()
    ns.ops, ns.Fn, ns.cp = ops, functional, cp
    return ns


def set_prec(ops, prec):
    if prec == "mixed":
        ops.reset_precision()
    else:
        ops.set_compute_dtype(prec)


def q16(x, dt):
    return x.to(dt).double()


def report(name, got, ref, tol):
    e = maxerr(got, ref)
    print("%-64s max|err| %.3e  rmse %.3e  tol %.1e" % (name, e, rmse(got, ref), tol))
    assert math.isfinite(e) and e <= tol, "%s: max err %.3e > %.1e" % (name, e, tol)


def make_pipe(pkg, sd, **model_kw):
    pipe = pkg.cp.ConformerPipeline()
    pipe.model = pkg.cp.SpeechEnhancer(**(model_kw or dict(n_freq=129)))
    pipe.model.load_state_dict(sd, strict=True)
    pipe.model = pipe.model.cuda().eval()
    return pipe


def run_packed(pkg, pipe, sigs, max_frames=None):
    """[(enh_real, enh_imag, mask_mag, wave)] per signal (CPU tensors / numpy) from packed passes"""
    out = []
    with torch.no_grad():
        for seg in pkg.Fn.packed_segments([w.size for w in sigs], max_frames=max_frames):
            x = torch.from_numpy(np.concatenate(sigs[seg.start:seg.stop])).cuda()
            nr, ni = pkg.Fn.stft_packed(x, seg)
            er, ei, mm = pipe.model.forward_packed(nr, ni, seg)
            y = pkg.Fn.istft_packed(er, ei, seg).cpu()
            cut = lambda t: t.cpu().split(seg.frame_counts.tolist(), dim=0)
            for i, parts in enumerate(zip(cut(er), cut(ei), cut(mm))):
                out.append(parts + (y[seg.sample_offsets[i]:seg.sample_offsets[i + 1]].numpy(),))
    return out


# ---------------------------------------------------------------------------
# 1. the path against the oracle on every utterance alone
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference():
    sigs, sd = rc.waves(), rc.enhancer_state()
    return sigs, sd, rc.oracle_alone(sd, sigs)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_packed_path_matches_the_oracle_on_every_utterance(pkg, reference, prec):
    sigs, sd, ref = reference
    set_prec(pkg.ops, prec)
    pipe = make_pipe(pkg, sd)
    got = run_packed(pkg, pipe, sigs)
    waves = pipe.enhance_batch(sigs)
    assert [w.shape for w in waves] == [(n,) for n in rc.LENGTHS] and all(w.dtype == np.float32 for w in waves)
    bad = []
    for i, (g, r) in enumerate(zip(got, ref)):
        m, wv = rmse(g[2], r[4]), rel_rmse(waves[i], r[5])
        print("packed %-5s L %5d T %3d | mask RMSE %.3e (bound %.0e) | wave rel RMSE %.3e (bound %.0e)" % (
            prec, rc.LENGTHS[i], rc.FRAMES[i], m, HARD_BOUND[prec], wv, WAVE_BOUND[prec]))
        assert np.array_equal(waves[i], g[3])                       # enhance_batch is the same pass
        if not (m <= HARD_BOUND[prec] and wv < WAVE_BOUND[prec]):
            bad.append((i, m, wv))
    assert not bad, bad


@pytest.mark.parametrize("prec", PRECISIONS)
def test_packed_path_at_the_reference_test_size(pkg, prec):
    """d_model 64, 4 heads, d_ff 128, k 7, 2 blocks: the generic attention kernel (head_dim 16) and the k 7 depthwise kernel"""
    sigs, sd = rc.waves(), rc.small_state()
    ref = rc.oracle_alone(sd, sigs)
    set_prec(pkg.ops, prec)
    pipe = make_pipe(pkg, sd, **rc.SMALL)
    got = run_packed(pkg, pipe, sigs)
    bad = []
    for i, (g, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("enh_real", "enh_imag", "mask_mag"), g[:3], r[2:5]):
            e = rel_rmse(a, b)
            print("small %-5s T %3d %-8s rel RMSE %.3e (bound %.0e)" % (prec, rc.FRAMES[i], name, e, WIDTH_EVAL_TOL[prec]))
            if not e < WIDTH_EVAL_TOL[prec]:
                bad.append((i, name, e))
    assert not bad, bad


@pytest.mark.parametrize("shape", [dict(d_model=192, num_heads=4, d_ff=768, kernel_size=15),        # hd 48, generic depthwise
                                   dict(d_model=384, num_heads=6, d_ff=1536, kernel_size=31),       # hd 64 at H 6, C 384
                                   dict(d_model=256, num_heads=8, d_ff=1024, kernel_size=31)])      # hd 32, fused FFN
def test_other_widths_run_packed_and_match_their_dense_forward(pkg, shape):
    """every configuration the dense eval forward takes runs packed: same bound as the dense forward against the oracle"""
    from sincformer_metacog_speech_enhancement_amd import synthetic as syn
    kw = dict(n_freq=129, num_blocks=2, dropout=0.0, **shape)
    shapes = {k: tuple(v.shape) for k, v in pkg.cp.SpeechEnhancer(**kw).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes, 34).items()}
    sigs = rc.waves()
    ref = rc.oracle_alone(sd, sigs, shape["num_heads"])
    pkg.ops.reset_precision()
    got = run_packed(pkg, make_pipe(pkg, sd, **kw), sigs)
    for i, (g, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("enh_real", "enh_imag", "mask_mag"), g[:3], r[2:5]):
            e = rel_rmse(a, b)
            print("D%d H%d k%d T %3d %-8s rel RMSE %.3e" % (shape["d_model"], shape["num_heads"], shape["kernel_size"], rc.FRAMES[i], name, e))
            assert e < WIDTH_EVAL_TOL["mixed"], (i, name, e)


# ---------------------------------------------------------------------------
# 2. independence of the company
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_a_signal_gets_bitwise_the_same_result_in_any_company(pkg, reference, prec):
    """same signals, other order: same M, so the same kernel routing; every row-wise kernel computes a row from that row alone
    and the packed kernels anchor their tiles at the utterance start"""
    sigs, sd, _ = reference
    set_prec(pkg.ops, prec)
    pipe = make_pipe(pkg, sd)
    base = run_packed(pkg, pipe, sigs)
    n = len(sigs)
    for name, perm in (("reversed", list(range(n))[::-1]), ("rotated by 3", [(i + 3) % n for i in range(n)])):
        got = run_packed(pkg, pipe, [sigs[j] for j in perm])
        waves = pipe.enhance_batch([sigs[j] for j in perm])
        for k, j in enumerate(perm):
            for part, a, b in zip(("enh_real", "enh_imag", "mask_mag"), got[k][:3], base[j][:3]):
                assert torch.equal(a, b), (name, j, part)
            assert np.array_equal(got[k][3], base[j][3]) and np.array_equal(waves[k], base[j][3]), (name, j, "wave")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_alone_split_and_dense_agree_with_the_one_pass_result(pkg, reference, prec):
    """a batch of one signal, enhance_signal on it, and a max_frames split: different M may route to different GEMM kernels,
    so not bitwise - within the bounds of the path test"""
    sigs, sd, _ = reference
    set_prec(pkg.ops, prec)
    pipe = make_pipe(pkg, sd)
    base = run_packed(pkg, pipe, sigs)
    split = run_packed(pkg, pipe, sigs, max_frames=60)
    assert [w.size for w in pipe.enhance_batch(sigs, max_frames=60)] == rc.LENGTHS
    for i, w in enumerate(sigs):
        alone = run_packed(pkg, pipe, [w])[0]
        dense = pipe.enhance_signal(w)
        figs = dict(alone_mask=rmse(alone[2], base[i][2]), split_mask=rmse(split[i][2], base[i][2]),
                    alone_wave=rel_rmse(alone[3], base[i][3]), split_wave=rel_rmse(split[i][3], base[i][3]),
                    dense_wave=rel_rmse(dense, base[i][3]))
        print("T %3d %s | " % (rc.FRAMES[i], prec) + "  ".join("%s %.2e" % kv for kv in figs.items()))
        assert figs["alone_mask"] <= HARD_BOUND[prec] and figs["split_mask"] <= HARD_BOUND[prec]
        assert max(figs["alone_wave"], figs["split_wave"], figs["dense_wave"]) < WAVE_BOUND[prec]


# ---------------------------------------------------------------------------
# 3. kernel level
# ---------------------------------------------------------------------------
def _tables(pkg, T, H=None, lengths=None):
    seg = pkg.Fn.PackedSegments(T, lengths)
    return seg, seg.tables(torch.device("cuda"), H)


def _attn_ref64(qkv, T, H, hd):
    """float64 softmax(Q K^T / sqrt(hd)) V of every utterance by itself, rows back to back"""
    D = H * hd
    out = []
    for x in qkv.split(list(T), dim=0):
        q, k, v = [p.reshape(-1, H, hd).transpose(0, 1) for p in x.split(D, dim=-1)]
        p = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
        out.append((p @ v).transpose(0, 1).reshape(-1, D))
    return torch.cat(out)


def _attention_case(pkg, dt, T, H, hd, seed, scale, odt=None):
    pkg.ops.set_compute_dtype(dt)
    seg, tb = _tables(pkg, T, H if hd == 64 else None)
    qkv = arr("aq", (seg.sum_T, 3 * H * hd), seed, scale)
    out = pkg.ops.attention_varlen(qkv.cuda().to(dt).contiguous(), tb["frame_off"], tb["attn_items", H] if hd == 64 else None,
                                   seg.B, seg.max_T, seg.sum_T, H, hd, out_dtype=odt)
    assert out.dtype == (odt or dt)
    return out.float().cpu(), _attn_ref64(q16(qkv, dt), T, H, hd)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("T", [MIXED_T, ONE_T, [200, 200, 200]], ids=["mixed", "one", "equal"])
def test_attention_varlen_hd64(pkg, dt, H, T):
    got, ref = _attention_case(pkg, dt, T, H, 64, 40 + len(T), 1.5)
    report("attention varlen %s H%d T%s" % (dt, H, T[:6]), got, ref, 6 * EPS[dt])
    if len(set(T)) == 1:                                   # all lengths equal: the dense entry point, same reference, same bound
        pkg.ops.set_compute_dtype(dt)
        qkv = arr("aq", (sum(T), 3 * H * 64), 40 + len(T), 1.5)
        dense = pkg.ops.attention(qkv.cuda().to(dt).contiguous(), len(T), T[0], H, 64)
        report("attention dense twin %s H%d" % (dt, H), dense.float().cpu(), ref, 6 * EPS[dt])


def test_attention_varlen_more_items_than_cus(pkg):
    T = many_T()
    got, ref = _attention_case(pkg, torch.bfloat16, T, 4, 64, 91, 1.0)
    assert pkg.ops.attention_items(T, 4).shape[0] > 4 * 256
    report("attention varlen 300 utterances", got, ref, 6 * EPS[torch.bfloat16])


def test_attention_varlen_result_in_the_other_16bit_format(pkg):
    for dt, odt in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        got, ref = _attention_case(pkg, dt, MIXED_T, 4, 64, 92, 1.0, odt=odt)
        report("attention varlen %s -> %s" % (dt, odt), got, ref, 6 * max(EPS[dt], EPS[odt]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,hd", [(4, 16), (4, 48), (2, 128)])
@pytest.mark.parametrize("T", [MIXED_T, ONE_T, [150, 150]], ids=["mixed", "one", "equal"])
def test_attention_varlen_generic_kernel(pkg, dt, H, hd, T):
    got, ref = _attention_case(pkg, dt, T, H, hd, 40 + len(T), 1.5)
    report("attention varlen generic %s H%d hd%d T%s" % (dt, H, hd, T[:6]), got, ref, 6 * EPS[dt])
    with pytest.raises(RuntimeError, match="unsupported shape"):      # as the dense twin: the operands' format only
        _attention_case(pkg, dt, T, H, hd, 1, 1.0, odt=torch.float16 if dt is torch.bfloat16 else torch.bfloat16)


def _dwconv_case(pkg, dt, C, KS, T):
    pkg.ops.set_compute_dtype(dt)
    seg, tb = _tables(pkg, T)
    x = arr("dx", (seg.sum_T, C), 60)
    w, b = arr("dw", (C, 1, KS), 61) / math.sqrt(KS), arr("db", (C,), 62) * 0.1
    bw, bb = arr("dbw", (C,), 63) * 0.1 + 1, arr("dbb", (C,), 64) * 0.1
    rm, rv = arr("drm", (C,), 65) * 0.1, torch.rand(C, generator=torch.Generator().manual_seed(1)) + 0.5
    sc = bw / torch.sqrt(rv + 1e-5)
    sh = bb - rm * sc + b * sc
    out = pkg.ops.dwconv_folded_varlen(x.cuda().to(dt).contiguous(), w.reshape(C, KS).t().contiguous().cuda(), sc.cuda(), sh.cuda(),
                                       tb["frame_off"], tb["conv_tiles"], seg.B, seg.max_T, seg.sum_T, C)
    ref = []
    for p in q16(x, dt).split(list(T), dim=0):
        h = F.conv1d(p.t().unsqueeze(0), w.double(), b.double(), padding=(KS - 1) // 2, groups=C)
        h = orc.batch_norm_eval(h, bw.double(), bb.double(), rm.double(), rv.double())
        ref.append(orc.swish(h)[0].t())
    return out.float().cpu(), torch.cat(ref), (x, w, sc, sh)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C,KS", [(256, 31), (64, 7), (192, 15)])
@pytest.mark.parametrize("T", [MIXED_T, ONE_T, [200, 200, 200]], ids=["mixed", "one", "equal"])
def test_dwconv_folded_varlen(pkg, dt, C, KS, T):
    got, ref, (x, w, sc, sh) = _dwconv_case(pkg, dt, C, KS, T)
    report("dwconv varlen %s C%d k%d T%s" % (dt, C, KS, T[:6]), got, ref, 8 * EPS[dt])
    if len(set(T)) == 1:
        dense = pkg.ops.dwconv_folded(x.cuda().to(dt).contiguous(), w.reshape(C, KS).t().contiguous().cuda(), sc.cuda(), sh.cuda(),
                                      len(T), T[0], C)
        report("dwconv dense twin %s C%d k%d" % (dt, C, KS), dense.float().cpu(), ref, 8 * EPS[dt])


def test_dwconv_folded_varlen_more_tiles_than_cus(pkg):
    got, ref, _ = _dwconv_case(pkg, torch.float16, 256, 31, many_T())
    report("dwconv varlen 300 utterances", got, ref, 8 * EPS[torch.float16])


# signal lengths: T = 2 (L 129 and 130, the shortest), L below n_fft, multiples of neither the hop nor 16, T = 128 / 129 (the row
# tile and tile + 1), one of 1101 frames next to 2-frame ones
STFT_L = [129, 1600, 1637, 130, 479, 200, 88000, 129, 10160, 10240]


def _stft_lengths(kind):
    if kind == "mixed":
        return STFT_L
    if kind == "one":
        return [1637]
    if kind == "equal":
        return [1600, 1600, 1600]
    return [80 * t + (7 * i) % 80 for i, t in enumerate(many_T())]


@pytest.mark.parametrize("split16", [False, True], ids=["fp32", "split16"])
@pytest.mark.parametrize("kind", ["mixed", "one", "equal", "many"])
def test_stft_packed(pkg, kind, split16):
    """every utterance framed from its own samples with the reflection at its own ends; the LAST frame of every utterance
    (the one a kernel that runs into the neighbour gets wrong) is held to the bound on its own"""
    pkg.ops.set_compute_dtype(torch.bfloat16)
    Ls = _stft_lengths(kind)
    (seg,) = pkg.Fn.packed_segments(Ls)
    x = arr("stx", (seg.sum_L,), 30, 0.3)
    re, im = pkg.Fn.stft_packed(x.cuda(), seg, split16=split16)
    got = torch.cat([re, im], -1).cpu().split(seg.frame_counts.tolist(), dim=0)
    ref = [torch.cat(dft64(frame64(xi.double().unsqueeze(0), rc.N_FFT, rc.HOP, rc.WIN), rc.N_FFT, rc.WIN), -1)[0] for xi in x.split(Ls)]
    rms = float(torch.cat(ref).pow(2).mean().sqrt())
    # the exact form: 2e-5 on max |err| (test_stft_istft); the split-bf16 form: its dense twin's 2e-5 x rms x 8 on max |err| and
    # 2e-5 x rms on the rmse over everything (test_stft_split16_vs_oracle)
    tol = 2e-5 * 8 * rms if split16 else 2e-5
    worst_last = 0.0
    for i in range(seg.B):
        e, last = maxerr(got[i], ref[i]), maxerr(got[i][-1], ref[i][-1])
        worst_last = max(worst_last, last / tol)
        assert e <= tol and last <= tol, ("utterance %d L %d" % (i, Ls[i]), e, last, tol)
    if split16:
        assert rmse(torch.cat(got), torch.cat(ref)) < 2e-5 * rms
    print("stft packed %s %s: %d utterances, worst last-frame error %.2f of the bound" % (kind, "split16" if split16 else "fp32",
                                                                                          len(Ls), worst_last))
    if kind == "equal" and not split16:
        dr, di = pkg.Fn.stft(x.reshape(3, 1600).cuda())
        assert torch.equal(dr.reshape(-1, 129), re) and torch.equal(di.reshape(-1, 129), im)       # a row depends on its samples only


@pytest.mark.parametrize("kind", ["mixed", "one", "equal", "many"])
def test_istft_packed(pkg, kind):
    """per-utterance frame range, envelope and length; the last n_fft/2 samples of every utterance on their own"""
    pkg.ops.set_compute_dtype(torch.bfloat16)
    Ls = _stft_lengths(kind)
    (seg,) = pkg.Fn.packed_segments(Ls)
    pr, pi = arr("isr", (seg.sum_T, 129), 31, 0.3), arr("isi", (seg.sum_T, 129), 32, 0.3)
    y = pkg.Fn.istft_packed(pr.cuda(), pi.cuda(), seg).cpu()
    assert y.shape == (seg.sum_L,)
    worst = 0.0
    for i, (a, b, yi) in enumerate(zip(pr.split(seg.frame_counts.tolist()), pi.split(seg.frame_counts.tolist()), y.split(Ls))):
        ref = istft64(a.double().unsqueeze(0), b.double().unsqueeze(0), Ls[i], rc.N_FFT, rc.HOP, rc.WIN)[0]
        e, tail = maxerr(yi, ref), maxerr(yi[-128:], ref[-128:])
        worst = max(worst, e)
        assert e <= 2e-5 and tail <= 2e-5, ("utterance %d L %d" % (i, Ls[i]), e, tail)
    print("istft packed %s: %d utterances, max|err| %.3e (bound 2e-5)" % (kind, len(Ls), worst))
    if kind == "equal":
        dense = pkg.Fn.istft(pr.reshape(3, -1, 129).cuda(), pi.reshape(3, -1, 129).cuda(), 1600).cpu()
        report("istft dense twin", dense.reshape(-1), torch.cat([istft64(a.double().unsqueeze(0), b.double().unsqueeze(0), 1600,
               rc.N_FFT, rc.HOP, rc.WIN)[0] for a, b in zip(pr.split(21), pi.split(21))]), 2e-5)


@pytest.mark.parametrize("entry", ["attention hd64", "attention generic", "dwconv k31", "dwconv generic", "stft", "stft split16", "istft"])
def test_kernels_give_an_utterance_bitwise_the_same_rows_in_any_company(pkg, entry):
    """kernel-level form of the independence check, for each new entry point: utterance lists in two orders"""
    pkg.ops.set_compute_dtype(torch.float16)
    T = [5, 300, 1, 129, 64, 2, 131]
    perm = [3, 0, 6, 1, 5, 2, 4]
    if entry in ("stft", "stft split16", "istft"):
        Ls = [80 * t + 3 * i + 50 for i, t in enumerate(T)]
        x = arr("stx", (sum(Ls),), 30, 0.3).split(Ls)
        spec = arr("isr", (sum(1 + n // 80 for n in Ls), 258), 31, 0.3).split([1 + n // 80 for n in Ls])

        def run(order):
            (seg,) = pkg.Fn.packed_segments([Ls[j] for j in order])
            if entry == "istft":
                s = torch.cat([spec[j] for j in order]).cuda()
                return pkg.Fn.istft_packed(s[:, :129], s[:, 129:], seg).cpu().split([Ls[j] for j in order])
            re, im = pkg.Fn.stft_packed(torch.cat([x[j] for j in order]).cuda(), seg, split16=entry.endswith("16"))
            return torch.cat([re, im], -1).cpu().split(seg.frame_counts.tolist())
    else:
        H, hd, C, KS = (4, 64, 256, 31) if entry in ("attention hd64", "dwconv k31") else (4, 16, 192, 15)
        width = 3 * H * hd if entry.startswith("attention") else C
        rows = arr("aq", (sum(T), width), 50, 1.0).split(T)
        wT, sc, sh = arr("dw", (KS, C), 61).cuda() / math.sqrt(KS), (arr("dbw", (C,), 63) * 0.1 + 1).cuda(), (arr("dbb", (C,), 64) * 0.1).cuda()

        def run(order):
            seg, tb = _tables(pkg, [T[j] for j in order], H if hd == 64 else None)
            xin = torch.cat([rows[j] for j in order]).cuda().half().contiguous()
            if entry.startswith("attention"):
                o = pkg.ops.attention_varlen(xin, tb["frame_off"], tb["attn_items", H] if hd == 64 else None, seg.B, seg.max_T,
                                             seg.sum_T, H, hd)
            else:
                o = pkg.ops.dwconv_folded_varlen(xin, wT, sc, sh, tb["frame_off"], tb["conv_tiles"], seg.B, seg.max_T, seg.sum_T, C)
            return o.cpu().split([T[j] for j in order])
    base, other = run(list(range(len(T)))), run(perm)
    for k, j in enumerate(perm):
        assert torch.equal(other[k], base[j]), (entry, "utterance", j)


# ---------------------------------------------------------------------------
# 4. guards and launch structure
# ---------------------------------------------------------------------------
def test_forward_packed_is_loud_outside_inference(pkg, reference):
    sigs, sd, _ = reference
    pipe = make_pipe(pkg, sd)
    nr = torch.zeros(5, 129, device="cuda")
    pipe.model.train()
    with pytest.raises(RuntimeError, match="inference"):
        pipe.model.forward_packed(nr, nr, [2, 3])
    pipe.model.eval()
    with pytest.raises(RuntimeError, match="inference"):
        pipe.model.forward_packed(nr.clone().requires_grad_(True), nr, [2, 3])
    with pytest.raises(RuntimeError, match="sum of the frame counts"):
        with torch.no_grad():
            pipe.model.forward_packed(nr, nr, [2, 2])
    with pytest.raises(ValueError, match="signal 1"):
        pipe.enhance_batch([sigs[0], sigs[0][:100]])
    assert pipe.enhance_batch([]) == []
    with torch.no_grad():
        out = pipe.model.forward_packed(nr, nr, [2, 3])
    assert [tuple(t.shape) for t in out] == [(5, 129)] * 3
    wide = pkg.cp.SpeechEnhancer(n_freq=129, d_model=512, num_blocks=1, num_heads=1, d_ff=64, kernel_size=7).cuda().eval()
    with pytest.raises(NotImplementedError, match="d_model 512 with 1 heads"):
        with torch.no_grad():
            wide.forward_packed(nr, nr, [2, 3])


def _launches(ops, fn):
    ops.profiler.enable(None)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in ops.profiler.records]
    finally:
        ops.profiler.disable()
        ops.profiler.records = []


def test_a_pass_launches_the_same_kernels_for_1_7_and_40_utterances(pkg, reference):
    """nothing in a packed pass loops over utterances on the host"""
    sigs, sd, _ = reference
    pkg.ops.reset_precision()
    pipe = make_pipe(pkg, sd)
    forty = [np.concatenate([sigs[i % 7], sigs[(i + 1) % 7][:13 * (i // 7)]]) for i in range(40)]
    lists = [_launches(pkg.ops, lambda s=s: pipe.enhance_batch(s)) for s in ([sigs[3]], sigs, forty)]
    assert lists[0] == lists[1] == lists[2], lists
    assert lists[0].count("attention_fwd_varlen") == 4 and lists[0].count("dwconv_varlen") == 4
    assert lists[0].count("framed_gemm_f32_varlen") == 1 and lists[0].count("istft_ola_varlen") == 1
    assert "attention_fwd" not in lists[0] and "dwconv_bn_swish" not in lists[0] and "istft_ola" not in lists[0]
    assert len(lists[0]) < 80, len(lists[0])
