"""Training on packed rows, on the device: the three packed kernels (attention forward with LSE and dropout, attention backward,
depthwise weight gradient), the ConformerBlock training node with a PackedSegments, and SpeechEnhancer.forward_packed_train.
Cases, bounds and float64 references: tests/packed_train_cases.py (their own checks, and the wrong variants that must miss these
bounds, run without a GPU in tests/test_packed_train_host.py).  Needs a real MI355X: `pytest -m gpu`."""
import math

import pytest
import torch

import helpers as hp
import packed_train_cases as pc
from helpers import maxerr, rmse

pytestmark = pytest.mark.gpu
H, HD, D = pc.H, pc.HD, pc.D
IDS = {torch.float16: "f16", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dt", pc.DTYPES, ids=list(IDS.values()))


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from sincformer_metacog_speech_enhancement_amd import ops, functional, train
    from sincformer_metacog_speech_enhancement_amd.training import conformer_pipeline as cp

    class NS:
        pass
    ns = NS()
    ns.ops, ns.Fn, ns.train, ns.cp = ops, functional, train, cp
    yield ns
    ops.reset_precision()


def report(name, got, ref, tol):
    e = maxerr(got, ref)
    print("%-60s max|err| %.3e  rmse %.3e  tol %.1e" % (name, e, rmse(got, ref), tol))
    assert math.isfinite(e) and e <= tol, "%s: max err %.3e > %.1e" % (name, e, tol)


def _tables(pkg, lengths):
    seg = pkg.Fn.packed_frames(lengths)
    return seg, seg.tables(torch.device("cuda"), H)


def _attn_packed(pkg, name, dt, p, lse=None, delta=None):
    """the three packed attention results of a length set on the device: O, LSE [H, sum_T], dqkv"""
    ops = pkg.ops
    ops.set_compute_dtype(dt)
    seg, tb = _tables(pkg, pc.ATTN_SETS[name])
    qkv, dO = [t.cuda().to(dt).contiguous() for t in pc.attn_inputs(name, dt)]
    args = (tb["frame_off"], tb["attn_items", H], seg.B, seg.max_T, seg.sum_T, H, HD)
    O, lse = ops.attention_train_varlen(qkv, *args, p_drop=p, seed=pc.SEED, sum_T2=seg.sum_T2, lse=lse)
    dqkv = ops.attention_bwd_varlen(qkv, O, dO, lse, *args, p_drop=p, seed=pc.SEED, sum_T2=seg.sum_T2, delta=delta)
    return qkv, dO, O, lse, dqkv


# ---- 1. equals the dense launch -------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_equal_length_pack_is_the_dense_launch_bit_for_bit(pkg, dt, p):
    B, T = 3, 130
    qkv, dO, O, lse, dqkv = _attn_packed(pkg, "equal", dt, p)
    Od, lsed = pkg.ops.attention_train(qkv, B, T, H, HD, p_drop=p, seed=pc.SEED)
    dqkvd = pkg.ops.attention_bwd(qkv, Od, dO, lsed, B, T, H, HD, p_drop=p, seed=pc.SEED)
    assert torch.equal(O, Od)
    assert torch.equal(lse.view(H, B, T), lsed.permute(1, 0, 2))          # [H, sum_T] against [B, H, T]
    assert torch.equal(dqkv, dqkvd)
    if p > 0:                                                              # (and the mask is a mask: the p = 0 result differs)
        assert not torch.equal(O, _attn_packed(pkg, "equal", dt, 0.0)[2])


@dtypes
@pytest.mark.parametrize("name", ["ragged", "reversed"])
def test_every_utterance_of_a_ragged_pack_is_the_dense_launch_on_it_alone(pkg, dt, name):
    lengths = pc.ATTN_SETS[name]
    qkv, dO, O, lse, dqkv = _attn_packed(pkg, name, dt, 0.0)
    for u, T in enumerate(lengths):
        r = pc.rows_of(lengths, u)
        q1, d1 = qkv[r].contiguous(), dO[r].contiguous()
        O1, lse1 = pkg.ops.attention_train(q1, 1, T, H, HD)
        g1 = pkg.ops.attention_bwd(q1, O1, d1, lse1, 1, T, H, HD)
        assert torch.equal(O[r], O1), (name, u, T)
        assert torch.equal(lse[:, r], lse1[0]), (name, u, T)
        assert torch.equal(dqkv[r], g1), (name, u, T)


@dtypes
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_lse_and_delta_are_written_everywhere_inside_and_nowhere_beyond(pkg, dt, p):
    n, guard = sum(pc.ATTN_RAGGED), 256
    nan = lambda: torch.full((H * n + guard,), float("nan"), device="cuda")
    lse, delta = nan(), nan()
    _, _, O, lse_out, dqkv = _attn_packed(pkg, "ragged", dt, p, lse=lse, delta=delta)
    assert lse_out is lse
    for name, t in (("lse", lse), ("delta", delta)):
        assert not torch.isnan(t[:H * n]).any(), name
        assert torch.isnan(t[H * n:]).all(), name
    assert torch.isfinite(O.float()).all() and torch.isfinite(dqkv.float()).all()


# ---- 2. against float64 ---------------------------------------------------------------------------------------------------------
@dtypes
@pytest.mark.parametrize("name,p", [("ragged", 0.0), ("reversed", 0.0), ("equal", 0.1), ("ragged", 0.1)])
def test_packed_attention_against_float64_per_utterance(pkg, dt, name, p):
    """O, LSE and dq / dk / dv of every utterance within the dense kernels' bounds; at p 0.1 the reference takes its keep mask
    from the replica under the packed row-index rule"""
    lengths = pc.ATTN_SETS[name]
    _, _, O, lse, dqkv = _attn_packed(pkg, name, dt, p)
    O, lse, dqkv = O.float().cpu(), lse.cpu(), dqkv.float().cpu()
    ref = pc.attn_case(name, dt, p)
    worst = [0.0, 0.0, 0.0, 0.0]
    bad = []
    for u, T in enumerate(lengths):
        r = pc.rows_of(lengths, u)
        ro, rl, rg = ref[u]
        t_o, t_l, t_g, t_r = pc.attn_tols(dt, rg)
        figs = [maxerr(O[r], ro) / t_o, maxerr(lse[:, r], rl) / t_l,
                max(maxerr(dqkv[r][:, i * D:(i + 1) * D], rg[:, i * D:(i + 1) * D]) for i in range(3)) / t_g,
                rmse(dqkv[r], rg) / t_r]
        worst = [max(a, b) for a, b in zip(worst, figs)]
        if not all(math.isfinite(f) and f <= 1.0 for f in figs[:3]) or not figs[3] < 1.0:
            bad.append((u, T, figs))
    print("ATTN | %s %s p=%.2f | worst fraction of the bound over %d utterances: O %.2f LSE %.2f dq/dk/dv %.2f rmse(dqkv) %.2f" %
          (name, IDS[dt], p, len(lengths), *worst))
    assert not bad, bad


# ---- 3. depthwise weight gradient -----------------------------------------------------------------------------------------------
def _wgrad(pkg, x, dy, lengths, KS, dt):
    seg, tb = _tables(pkg, lengths)
    C = x.shape[1]
    return pkg.ops.dwconv_wgrad_varlen(x.cuda().to(dt).contiguous(), dy.cuda().contiguous(), tb["frame_off"], tb["wgrad_spans"],
                                       seg.B, seg.sum_T, C, KS)


def _check_wgrad(name, got, c):
    hp.check_row(name + " dw", got[0].cpu(), c["ref64"][0], c["ref32"][0], hp.K_SUM, c["dw_bound"])
    hp.check_row(name + " db", got[1].cpu(), c["ref64"][1], c["ref32"][1], hp.K_SUM, c["db_bound"])


@dtypes
@pytest.mark.parametrize("KS,C", pc.WGRAD_ROWS)
def test_packed_dwconv_wgrad(pkg, dt, KS, C):
    """against the float64 sum over utterances at the dense twin's bound (K_SUM x e32 or (sum_T + 2) 2^-24 sum|terms|); the same
    bits on every run; accumulates into dw / db when given"""
    pkg.ops.set_compute_dtype(dt)
    c = pc.wgrad_case(KS, C, dt)
    name = "dwconv_wgrad_varlen KS%d C%d %s" % (KS, C, IDS[dt])
    got = _wgrad(pkg, c["x"], c["dy"], pc.CONV_LENGTHS, KS, dt)
    again = _wgrad(pkg, c["x"], c["dy"], pc.CONV_LENGTHS, KS, dt)
    _check_wgrad(name, got, c)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    seg, tb = _tables(pkg, pc.CONV_LENGTHS)
    sw, sb = torch.full((C, KS), 3.0, device="cuda"), torch.full((C,), -2.0, device="cuda")
    acc = pkg.ops.dwconv_wgrad_varlen(c["x"].cuda().to(dt).contiguous(), c["dy"].cuda().contiguous(), tb["frame_off"],
                                      tb["wgrad_spans"], seg.B, seg.sum_T, C, KS, dw=sw.clone(), db=sb.clone())
    assert torch.equal(acc[0], sw + got[0]) and torch.equal(acc[1], sb + got[1])


@dtypes
@pytest.mark.parametrize("KS,C", pc.WGRAD_ROWS[:2])
def test_a_pack_of_one_utterance_is_the_dense_launch_within_the_bound(pkg, dt, KS, C):
    """not bitwise: the span cut may differ.  Both sides meet the one bound against the one float64 reference"""
    pkg.ops.set_compute_dtype(dt)
    T = 200
    x, dy = pc.wgrad_inputs([T], C, dt)
    c = pc.wgrad_ref(x, dy, [T], KS)
    _check_wgrad("pack of one KS%d %s" % (KS, IDS[dt]), _wgrad(pkg, x, dy, [T], KS, dt), c)
    dense = pkg.ops.dwconv_wgrad(x.cuda().to(dt).contiguous(), dy.cuda().contiguous(), 1, T, C, KS)
    _check_wgrad("dense B1 T%d KS%d %s" % (T, KS, IDS[dt]), dense, c)


@dtypes
@pytest.mark.parametrize("j", [0, 5, 11])
def test_perturbing_one_utterance_moves_the_result_by_its_own_contribution(pkg, dt, j):
    """nothing leaks across a boundary: with utterance j's x and dy replaced, the result is the old float64 sum minus j's old
    contribution plus its new one, within the bound"""
    pkg.ops.set_compute_dtype(dt)
    KS, C = 31, 256
    c = pc.wgrad_case(KS, C, dt)
    r = pc.rows_of(pc.CONV_LENGTHS, j)
    x2, dy2 = c["x"].clone(), c["dy"].clone()
    nx, ndy = pc.wgrad_inputs([pc.CONV_LENGTHS[j]], C, dt, tag=100 + j)
    x2[r], dy2[r] = nx * 0.5, ndy - 4.0
    old = pc.wgrad_ref(c["x"][r], c["dy"][r], [pc.CONV_LENGTHS[j]], KS)["ref64"]
    new = pc.wgrad_ref(x2[r], dy2[r], [pc.CONV_LENGTHS[j]], KS)["ref64"]
    c2 = pc.wgrad_ref(x2, dy2, pc.CONV_LENGTHS, KS)
    moved = (c["ref64"][0] - old[0] + new[0], c["ref64"][1] - old[1] + new[1])
    assert hp.figs(moved[0], c2["ref64"][0])[1] < 1e-12 and hp.figs(moved[1], c2["ref64"][1])[1] < 1e-12
    c2["ref64"] = moved
    _check_wgrad("utterance %d perturbed %s" % (j, IDS[dt]), _wgrad(pkg, x2, dy2, pc.CONV_LENGTHS, KS, dt), c2)


# ---- 5 - 7. the block's training node -------------------------------------------------------------------------------------------
def _run_block(pkg, name, rows, p, bn_eval, seg=None, shape=None, seed=4242):
    """ConformerBlockFunction forward + backward on rows `rows` of the case's x / dy (seg: packed; shape: the dense [B, T, D])
    -> dict(out, dx, grads {name: fp32}, running (mean, var, batches))"""
    train = pkg.train
    sd, x, dy = pc.block_inputs(name)
    params = [sd[k].cuda().clone().requires_grad_(True) for k in train.PARAM_NAMES]
    buffers = tuple(sd["conv.batch_norm." + k].cuda().clone() for k in ("running_mean", "running_var", "num_batches_tracked"))
    xg, dyg = x[rows].cuda(), dy[rows].cuda()
    if shape is not None:
        xg, dyg = xg.reshape(shape), dyg.reshape(shape)
    xg = xg.contiguous().requires_grad_(True)
    meta = (H, p, seed, buffers, 0.1, 1e-5, bn_eval) + (() if seg is None else (seg,))
    y = train.ConformerBlockFunction.apply(xg, meta, *params)
    y.backward(dyg.contiguous())
    return dict(out=y.detach().reshape(-1, D), dx=xg.grad.reshape(-1, D), grads={k: t.grad for k, t in zip(train.PARAM_NAMES, params)},
                running=buffers)


DEPTHWISE = ("conv.depthwise.weight", "conv.depthwise.bias")
# a gradient that is analytically zero has no relative error: max|g| is held to this fraction of max|g| of its sibling, the
# bound tests/test_train_gpu.py::test_block_train_forward_backward_matches_autograd holds the dense block's depthwise bias to
ZERO_TOL = 1e-3


@dtypes
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_block_on_an_equal_length_pack_is_the_dense_block(pkg, dt, p, monkeypatch):
    """[130, 130, 130], BatchNorm batch statistics: output, dx, every parameter gradient but the depthwise pair and the updated
    running statistics bit for bit; the depthwise pair meets the weight-gradient bound against float64 of the operands it was
    handed (recorded from the call)"""
    ops = pkg.ops
    ops.set_compute_dtype(dt)
    lengths = pc.ATTN_SETS["equal"]
    seg = pkg.Fn.packed_frames(lengths)
    seen = []
    real = ops.dwconv_wgrad_varlen

    def spy(x16, dy32, *a, **k):
        seen.append((x16.float().cpu(), dy32.cpu()))
        return real(x16, dy32, *a, **k)
    monkeypatch.setattr(ops, "dwconv_wgrad_varlen", spy)
    every = slice(0, sum(lengths))
    a = _run_block(pkg, "equal", every, p, False, seg=seg)
    b = _run_block(pkg, "equal", every, p, False, shape=(3, 130, D))
    assert len(seen) == 1
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dx"], b["dx"])
    for k in pkg.train.PARAM_NAMES:
        if k not in DEPTHWISE:
            assert torch.equal(a["grads"][k], b["grads"][k]), k
    for ra, rb in zip(a["running"], b["running"]):
        assert torch.equal(ra, rb)
    assert int(a["running"][2]) == 1
    c = pc.wgrad_ref(seen[0][0], seen[0][1], lengths, 31)
    for tag, r in (("packed", a), ("dense", b)):
        _check_wgrad("block depthwise gradients %s p=%.1f %s" % (tag, p, IDS[dt]),
                     (r["grads"][DEPTHWISE[0]].reshape(D, 31), r["grads"][DEPTHWISE[1]]), c)


@dtypes
@pytest.mark.parametrize("name", ["ragged", "reversed"])
def test_block_on_a_ragged_pack_with_frozen_batchnorm(pkg, dt, name):
    """bn_eval, p 0: every utterance's output and dx rows are the dense node's on [1, T_u] bit for bit; the parameter gradients
    match the float64 sum over utterances within the dense training path's relative RMSE"""
    pkg.ops.set_compute_dtype(dt)
    lengths = pc.ATTN_SETS[name]
    seg = pkg.Fn.packed_frames(lengths)
    a = _run_block(pkg, name, slice(0, sum(lengths)), 0.0, True, seg=seg)
    for u, T in enumerate(lengths):
        r = pc.rows_of(lengths, u)
        b = _run_block(pkg, name, r, 0.0, True, shape=(1, T, D))
        assert torch.equal(a["out"][r], b["out"]), (name, u, T)
        assert torch.equal(a["dx"][r], b["dx"]), (name, u, T)
    assert int(a["running"][2]) == 0                                        # frozen: the statistics did not move
    ref = pc.block_case(name, True)
    bad = []
    for k in pkg.train.PARAM_NAMES:
        e = hp.rel_rmse(a["grads"][k].cpu(), ref["grads"][k])
        print("BLOCK | %s %s bn_eval | d%-36s rel rmse %.3e (bound %.1e)" % (name, IDS[dt], k, e, pc.BLOCK_TOL[dt]))
        if not e <= pc.BLOCK_TOL[dt]:
            bad.append((k, e))
    assert not bad, bad


@dtypes
def test_block_on_a_ragged_pack_with_batch_statistics(pkg, dt):
    """p 0, statistics over all sum_T valid rows: output, dx, all parameter gradients and the running statistics against the
    float64 packed block.  conv.depthwise.bias is analytically zero here (BatchNorm removes the per-channel mean), so it has no
    relative error: it is held to ZERO_TOL of the depthwise weight gradient's size, as the dense test holds it."""
    pkg.ops.set_compute_dtype(dt)
    lengths = pc.ATTN_SETS["ragged"]
    a = _run_block(pkg, "ragged", slice(0, sum(lengths)), 0.0, False, seg=pkg.Fn.packed_frames(lengths))
    ref = pc.block_case("ragged", False)
    tol = pc.BLOCK_TOL[dt]
    figs = {"out": hp.rel_rmse(a["out"].cpu(), ref["out"]), "dx": hp.rel_rmse(a["dx"].cpu(), ref["dx"]),
            "running mean": hp.rel_rmse(a["running"][0].cpu(), ref["running"][0]),
            "running var": hp.rel_rmse(a["running"][1].cpu(), ref["running"][1])}
    for k in pkg.train.PARAM_NAMES:
        if k != "conv.depthwise.bias":
            figs["d" + k] = hp.rel_rmse(a["grads"][k].cpu(), ref["grads"][k])
    for k, e in figs.items():
        print("BLOCK | ragged %s batch statistics | %-38s rel rmse %.3e (bound %.1e)" % (IDS[dt], k, e, tol))
    zero = float(a["grads"]["conv.depthwise.bias"].abs().max()) / float(a["grads"]["conv.depthwise.weight"].abs().max())
    print("BLOCK | ragged %s batch statistics | dconv.depthwise.bias max|g| / max|d weight| %.3e (bound %.1e)" % (IDS[dt], zero, ZERO_TOL))
    assert int(a["running"][2]) == 1
    bad = [(k, e) for k, e in figs.items() if not e <= tol] + ([("dconv.depthwise.bias", zero)] if not zero <= ZERO_TOL else [])
    assert not bad, bad


# ---- 8. SpeechEnhancer.forward_packed_train -------------------------------------------------------------------------------------
# The mean over sum_T x F elements hands every element a cotangent of 1 / N = 4e-5, below fp16's smallest normal number (6e-5): the
# 16-bit cotangents of the GEMMs would be subnormals with two or three significant bits (gradients 2 - 3e-2 off, measured).  The
# step is scaled as fp16 training scales it (optim.DynamicLossScale, the reference's GradScaler): a power of two, exact to undo.
LOSS_SCALE = 4096.0


def _model(pkg, dt, p=None):
    pkg.ops.set_compute_dtype(dt)
    r = pc.MODEL_ROW
    m = pkg.cp.SpeechEnhancer(n_freq=r["n_freq"], d_model=r["d_model"], num_blocks=r["num_blocks"], num_heads=r["num_heads"],
                              d_ff=r["d_ff"], kernel_size=r["kernel_size"], dropout=r["p"] if p is None else p)
    m.load_state_dict(pc.model_state())
    return m.cuda()


def test_forward_packed_train_in_eval_is_forward_packed(pkg):
    """in the training format, fp16 (ops.TRAIN_DTYPE).  The 1e-3 mask bound is a bound of fp16 and mixed operands: the inference
    path in bf16 everywhere misses it against the reference on its own, and two bf16 routes to one mask
    differ by several 8-bit roundings (5e-3 here)"""
    dt = torch.float16
    m = _model(pkg, dt).eval()
    nr, ni = [t.cuda() for t in pc.model_inputs()[:2]]
    with torch.no_grad():
        want = m.forward_packed(nr, ni, pc.MODEL_LENGTHS)
    m.enable_eval_autograd()
    got = m.forward_packed_train(nr, ni, pc.MODEL_LENGTHS)
    assert got[0].requires_grad and got[1].requires_grad and not got[2].requires_grad
    for name, g, w in zip(("enh_real", "enh_imag", "mask_mag"), got, want):
        assert g.shape == w.shape == (sum(pc.MODEL_LENGTHS), pc.MODEL_ROW["n_freq"])
        report("forward_packed_train eval %s %s" % (IDS[dt], name), g.detach().cpu(), w.cpu(), pc.MASK_TOL)
    assert all(int(b.conv.batch_norm.num_batches_tracked) == 0 for b in m.blocks)
    ref = pc.model_case(True)
    for name, g, w in zip(("enh_real", "enh_imag", "mask_mag"), got, ref["out"]):
        print("MODEL | eval %s | %s rel rmse to float64 %.3e" % (IDS[dt], name, hp.rel_rmse(g.detach().cpu(), w)))


@dtypes
@pytest.mark.parametrize("frozen", [False, True], ids=["batch-statistics", "frozen-batchnorm"])
def test_one_packed_step_on_the_l1_magnitude_term(pkg, dt, frozen):
    """finite gradients for every parameter, within the block bounds of the float64 packed enhancer; p = 0 (the masks of a
    step are pinned at block level).  frozen: eval() with enable_eval_autograd(), BatchNorm on its running statistics.
    Two gradients are analytically zero and have no relative error: the phase head's (|enh| = mask_mag |noisy| whatever the
    phase) and, under batch statistics, the depthwise bias (BatchNorm removes the channel mean).  Each is held to ZERO_TOL of
    its sibling's size (the magnitude head, the depthwise weight), as the dense block test holds the bias."""
    m = _model(pkg, dt, p=0.0)
    if frozen:
        m.eval().enable_eval_autograd()
    else:
        m.train()
    nr, ni, cr, ci = [t.cuda() for t in pc.model_inputs()]
    er, ei, mm = m.forward_packed_train(nr, ni, pc.MODEL_LENGTHS)
    loss = pkg.train.L1MagnitudeFunction.apply(er, ei, cr, ci)
    (loss * LOSS_SCALE).backward()
    ref = pc.model_case(frozen)
    print("MODEL | %s %s | loss %.6f, float64 %.6f" % (IDS[dt], "frozen" if frozen else "batch statistics", float(loss), ref["loss"]))
    assert abs(float(loss) - ref["loss"]) <= pc.BLOCK_TOL[dt] * abs(ref["loss"])
    named = dict(m.named_parameters())
    bad = []
    for k, g64 in ref["grads"].items():
        assert named[k].grad is not None and torch.isfinite(named[k].grad).all(), k
        g = named[k].grad / LOSS_SCALE
        tol = ZERO_TOL
        if k.endswith("conv.depthwise.bias") and not frozen:                # analytically zero under batch statistics
            e = float(named[k].grad.abs().max()) / float(named[k.replace("bias", "weight")].grad.abs().max())
        elif k.startswith("phase_head."):                                   # analytically zero for a magnitude objective
            e = float(named[k].grad.abs().max()) / float(named[k.replace("phase", "mag")].grad.abs().max())
        else:
            e, tol = hp.rel_rmse(g.cpu(), g64), pc.BLOCK_TOL[dt]
        print("MODEL | %s %s | d%-44s %s %.3e (bound %.1e)" % (IDS[dt], "frozen" if frozen else "batch", k,
                                                             "rel rmse" if tol != ZERO_TOL else "max|g| / max|sibling|", e, tol))
        if not e <= tol:
            bad.append((k, e))
    assert not bad, bad


def test_a_repeated_set_of_lengths_neither_copies_nor_synchronises(pkg):
    """forward and backward of a second step on the same lengths (the backward reads the segment tables too)"""
    m = _model(pkg, torch.float16).train()
    nr, ni = [t.cuda() for t in pc.model_inputs()[:2]]
    cot = torch.ones_like(nr)

    def step(lengths):
        er, ei, mm = m.forward_packed_train(nr, ni, lengths)
        torch.autograd.backward([er, ei], [cot, cot])
        return er, ei, mm
    step(pc.MODEL_LENGTHS)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        er, ei, mm = step(list(pc.MODEL_LENGTHS))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(er).all() and torch.isfinite(ei).all() and torch.isfinite(mm).all()
    assert all(p_.grad is not None and torch.isfinite(p_.grad).all() for p_ in m.parameters())


@dtypes
def test_block_forward_packed_in_eval_runs_the_inference_kernels(pkg, dt):
    """ConformerBlock.forward_packed in eval() without autograd: functional.block_forward with the segments, bit for bit, no
    graph; and each utterance's rows are what the block's forward() gives that utterance alone, within the block bound"""
    pkg.ops.set_compute_dtype(dt)
    lengths = pc.ATTN_SETS["ragged"]
    sd, x, _ = pc.block_inputs("ragged")
    from sincformer_metacog_speech_enhancement_amd.models.conformer import ConformerBlock
    blk = ConformerBlock(D, H, pc.FF, 31, 0.1)
    blk.load_state_dict(sd)
    blk = blk.cuda().eval()
    xg = x.cuda()
    y = blk.forward_packed(xg, lengths)
    assert y.shape == xg.shape and not y.requires_grad and y.grad_fn is None
    pk = pkg.Fn.pack_block({k: v.detach() for k, v in blk.state_dict().items()}, H)
    want = pkg.Fn.block_forward(xg.float().contiguous(), pk, None, None, H, seg=pkg.Fn.packed_frames(lengths))
    assert torch.equal(y, want)
    with torch.no_grad():
        alone = torch.cat([blk(xg[pc.rows_of(lengths, u)][None])[0] for u in range(len(lengths))])
    e = hp.rel_rmse(y.cpu(), alone.cpu())
    print("BLOCK | eval forward_packed %s | rel rmse to forward() on each utterance alone %.3e (bound %.1e)" % (IDS[dt], e, pc.BLOCK_TOL[dt]))
    assert e <= pc.BLOCK_TOL[dt]
    assert int(blk.conv.batch_norm.num_batches_tracked) == int(sd["conv.batch_norm.num_batches_tracked"])
