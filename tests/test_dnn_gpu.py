"""SpeechEnhancementDNN on the device (csrc/dnn.hip, models/dnn.py, train.DnnFunction) against the float64 restatement of
tests/dnn_cases.py.  Needs a real MI355X: `pytest -m gpu`.

Bounds, none of them taken from the kernels:
  one layer      the kernel is handed 16-bit-exact operands, so float64 on them differs from it by fp32 accumulation and the result's
                 rounding only.  Every element: |d| <= K u S (u = 2^-24, S = |A| |W|^T + |b|: the worst case of any summation order),
                 RMS: <= 4 sqrt(K) u S (its probabilistic form, constant 4); behind the sigmoid both shrink by sigmoid' <= 1/4 and
                 2e-6 is added (v_exp_f32 on x log2(e) rounded to fp32: <= 4e-7 for |x| <= 20, the division 6e-8); a 16-bit result
                 adds half a unit in the last place of the value (2^-11 |v| + 2^-25 in fp16, 2^-8 |v| in bf16).
  model, context device minus exact float64, RMS and max, <= 4 x the same error of the operand-rounding emulation (computed here, on the
                 CPU): the factor tests/test_adversarial_gpu.py uses, for fp32 accumulation order and 16-bit roundings that fall the
                 other way.
  gradients      relative RMSE to a float64 backward that takes its active-and-kept masks from the device's saved activations
                 (h > 0) <= 4 x the emulation's.
  signs          share of hidden units whose sign differs from float64's `z > 0 and kept` <= 1e-3 (a condition, not a measurement;
                 the emulation alone gives 1.2e-4: tests/test_dnn_host.py), in fp16, the training format.
Each case prints its figures before it asserts (profiles/README.md records them)."""
import math
import os

import numpy as np
import pytest
import torch

import dnn_cases as dn
import dropout_cases as dc

pytestmark = pytest.mark.gpu

FMTS = {"f16": torch.float16, "bf16": torch.bfloat16}
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
U32 = 2.0 ** -24
R = 128                                                     # the kernel's row tile (ops.DNN_ROW_TILE)
MS = (1, R - 1, R, R + 1, 2 * R + 3)
SHAPES = ((594, 1024), (162, 64), (1024, 64), (1024, 130), (64, 64))
CTX_OF = {594: (54, 5), 162: (54, 1), 1024: (1024, 0), 64: (64, 0)}        # K = D (2 ctx + 1)
NAN = float("nan")


@pytest.fixture(scope="module")
def mods():
    from sincformer_metacog_speech_enhancement_amd import models, ops, train, training
    from sincformer_metacog_speech_enhancement_amd.signal_processing import FeatureExtractor
    assert ops.DNN_ROW_TILE == R
    return {"ops": ops, "models": models, "train": train, "training": training, "fe": FeatureExtractor()}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def saved(y):
    """what train.DnnFunction kept for the backward of y: (activations, fp32 output, fp32 weights)"""
    fn = y.grad_fn
    while not hasattr(fn, "saved"):
        fn = fn.next_functions[0][0]
    return fn.saved


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the layer kernel
# ---------------------------------------------------------------------------------------------------------------------------
def layer_bounds(S, v, K, fmt, out16, act):
    worst, typ = K * U32 * S, 4.0 * math.sqrt(K) * U32 * S
    if act == "sigmoid":
        worst, typ = worst / 4 + 2e-6, typ / 4 + 2e-6
    if out16:
        r = U16[fmt] * np.abs(v) + 2.0 ** -25
        worst, typ = worst + r, typ + r
    return worst, typ


def operand(mode, x16, M, K, dt, variant=0):
    """the device operand of rows 0 .. M of the 16-bit-exact matrix x16 (float64 [Mmax, K]), columns beyond K poisoned with nan
    wherever the contract lets the kernel not read them"""
    if mode == "rows16":
        K8 = (K + 7) // 8 * 8
        buf = torch.full((M, K8 + 8), NAN, device="cuda", dtype=dt)
        buf[:, :K8] = 0
        buf[:, :K] = dev(x16[:M], dt)
        return dict(a=buf)
    if mode == "rows32":
        if variant == 0:                                    # contiguous rows: 8-byte loads (every K here is even)
            return dict(a=dev(x16[:M]))
        buf = torch.full((M, K + 3), NAN, device="cuda")   # an odd row stride: 4-byte loads
        buf[:, :K] = dev(x16[:M])
        return dict(a=buf[:, :K])
    D, ctx = CTX_OF[K]                                      # one frame per utterance: the row is its raw row 2 ctx + 1 times
    return dict(a=dev(x16[:M, :D]).reshape(M, 1, D).contiguous(), context=ctx)


@pytest.mark.parametrize("mode", ["rows16", "rows32", "context"])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_layer(mods, fmt, K, N, mode):
    ops, dt = mods["ops"], FMTS[fmt]
    ops.set_compute_dtype(dt)
    Mmax = MS[-1]
    (W,), (b,) = dn.params((K, N), 100 + K + N)
    x = dn.rnd(dn.inputs(Mmax, K, 200 + K + N), dt)
    if mode == "context":
        D, ctx = CTX_OF[K]
        x = np.tile(x[:, :D], (1, 2 * ctx + 1))
    Wr = dn.rnd(W, dt)
    z = x @ Wr.T + b
    S = np.abs(x) @ np.abs(Wr).T + np.abs(b)
    pw = ops.pack_linear(dev(W), dev(b), k_pad_to=(K + 7) // 8 * 8)
    seed, p = 77, 0.2
    keep = dc.keep_elems(seed, 0, Mmax * N, p).reshape(Mmax, N)
    kept32 = np.float64(dc.inv_keep32(p))
    cases = (("relu", False, 0.0), ("relu", True, 0.0), ("sigmoid", True, 0.0), (None, False, 0.0), ("relu", False, p))
    for act, out_f32, pd in cases:
        want = {"relu": np.maximum(z, 0.0), "sigmoid": dn.sigmoid(z), None: z}[act]
        scale = np.where(keep > 0, kept32, 0.0) if pd > 0 else 1.0
        want = want * scale
        worst, typ = layer_bounds(S * scale, want, K, fmt, not out_f32, act)
        largest = None
        for M in reversed(MS):
            for variant in ((0, 1) if mode == "rows32" else (0,)):
                width = N if out_f32 else (N + 7) // 8 * 8 + 8
                out = torch.full((M, width), NAN, device="cuda", dtype=torch.float32 if out_f32 else dt)
                kw = operand(mode, x, M, K, dt, variant)
                ops.dnn_layer(pw=pw, act=act, out=out, p_drop=pd, seed=seed, **kw)
                again = torch.full_like(out, NAN)
                ops.dnn_layer(pw=pw, act=act, out=again, p_drop=pd, seed=seed, **kw)
                torch.cuda.synchronize()
                tag = "%s %s K%d N%d M%d act %s f32 %d p %.1f v%d" % (fmt, mode, K, N, M, act, out_f32, pd, variant)
                assert torch.equal(bits(out), bits(again)), tag                        # run to run
                got = host(out)
                assert np.isfinite(got).all(), tag                                     # every element written, no poison read
                assert (got[:, N:] == 0).all(), tag                                    # the pad columns are exactly 0
                d = np.abs(got[:, :N] - want[:M])
                if M == Mmax and variant == 0:
                    print("%s: max|d| %.3e (worst-case bound min %.3e)  rms %.3e (bound %.3e)"
                          % (tag, d.max(), worst.min(), dn.rms(d), dn.rms(typ)))
                    largest = bits(out)
                assert (d <= worst[:M]).all(), (tag, float((d - worst[:M]).max()))
                assert dn.rms(d) <= dn.rms(typ[:M]), (tag, dn.rms(d), dn.rms(typ[:M]))
                assert torch.equal(bits(out), largest[:M]), tag                        # a row alone or inside the largest M
                if pd > 0:
                    assert (got[:, :N][keep[:M] == 0] == 0).all(), tag


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_act_bwd(mods, fmt):
    """one pass, fp32 arithmetic in the order written in csrc/dnn.hip, one rounding to 16 bits: the bits are those of numpy's
    float32; N = 130 leaves 62 pad columns, which are exactly 0; M = 300 is more than one workgroup"""
    ops, dt = mods["ops"], FMTS[fmt]
    ops.set_compute_dtype(dt)
    M, N, p = 300, 130, 0.2
    rng = np.random.default_rng(41)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    h = np.maximum(rng.standard_normal((M, N)), 0.0).astype(np.float32)
    y = rng.random((M, N)).astype(np.float32)
    inv = dc.inv_keep32(p)
    for dy_dt in (torch.float32, dt):
        g = dev(dy, dy_dt)
        g32 = g.float().cpu().numpy()
        wide = torch.full((M, N + 6), NAN, device="cuda", dtype=dy_dt)                # a wider row stride, poisoned beyond N
        wide[:, :N] = g
        want = {"relu": np.where(dn.rnd(h, dt) > 0, g32 * inv, np.float32(0)), "sigmoid": (g32 * y) * (np.float32(1) - y), None: g32}
        for act, sv in (("relu", dev(h, dt)), ("sigmoid", dev(y)), (None, None)):
            out = torch.full((M, 192), NAN, device="cuda", dtype=dt)
            ops.dnn_act_bwd(wide[:, :N], sv, act, N, p_drop=p if act == "relu" else 0.0, out=out)
            dz = ops.dnn_act_bwd(g, sv, act, N, p_drop=p if act == "relu" else 0.0)
            torch.cuda.synchronize()
            assert dz.shape == (M, 192) and dz.dtype == dt and torch.equal(bits(out), bits(dz)), (act, dy_dt)
            assert (host(dz)[:, N:] == 0).all(), (act, dy_dt)
            assert torch.equal(bits(dz[:, :N]), bits(torch.from_numpy(want[act]).to(dt))), (act, dy_dt)


# ---------------------------------------------------------------------------------------------------------------------------
# the model: inference
# ---------------------------------------------------------------------------------------------------------------------------
def model(mods, case, fmt, dims):
    mods["ops"].set_compute_dtype(FMTS[fmt])
    m = mods["models"].SpeechEnhancementDNN(dims[0], dims[1], dims[-1], len(dims) - 2)
    m.load_state_dict(dn.state_dict(case["Ws"], case["bs"]))
    return m.cuda()


def check_forward(tag, got, exact, emulated):
    (r, m), (re, me) = dn.err(got, exact), dn.err(emulated, exact)
    print("%s: rms %.3e (emulation %.3e, ratio %.2f)  max %.3e (emulation %.3e, ratio %.2f)" % (tag, r, re, r / re, m, me, m / me))
    assert np.isfinite(got).all(), tag
    assert r <= 4.0 * re and m <= 4.0 * me, (tag, r, re, m, me)


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("which", ["default", "small"])
def test_model_forward(mods, which, fmt):
    case, dims = (dn.default_case(), dn.DEFAULT) if which == "default" else (dn.small_case(), dn.SMALL)
    m = model(mods, case, fmt, dims).eval()
    x = dev(case["x"])
    y = m(x)
    assert y.shape == (case["x"].shape[0], 64) and y.dtype == torch.float32 and not y.requires_grad
    y2 = m(x)
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(y2))
    check_forward("model %s %s M%d" % (which, fmt, x.shape[0]), host(y), case["y"], dn.emulation(case, FMTS[fmt])[0])
    assert torch.equal(bits(m(x.reshape(1, -1, 594))[0]), bits(y))                    # leading dimensions are rows
    if which == "small":
        golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_dnn.npz"))["y"]
        check_forward("model small %s against the fixture" % fmt, host(y), golden.astype(np.float64), dn.emulation(case, FMTS[fmt])[0])
    # eval() with autograd wanted runs the training node without dropout: the same value within the same bound
    ya = m(x.clone().requires_grad_(True))
    assert ya.requires_grad
    check_forward("model %s %s autograd node" % (which, fmt), host(ya), case["y"], dn.emulation(case, FMTS[fmt])[0])


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("with_stats", [False, True])
def test_context_mode(mods, with_stats, fmt):
    case = dn.small_case()
    m = model(mods, case, fmt, dn.SMALL).eval()
    raw, mean, std = dn.context_case()
    if not with_stats:
        raw = np.where(np.isfinite(raw), raw, 0.0).astype(np.float32)                # without statistics a nan stays a nan
        mean = std = None
    fe = mods["fe"]
    assert fe.context == dn.CTX
    stats = {} if mean is None else dict(feat_mean=dev(mean), feat_std=dev(std))
    for frames in (dn.CTX_FRAMES, (23, 0, 5), None):
        x = dn.context64(raw, frames, mean=mean, std=std).reshape(-1, 594)
        exact = dn.forward64(case["Ws"], case["bs"], x)[0]
        emu = dn.forward64(case["Ws"], case["bs"], x, fmt=FMTS[fmt])[0]
        y = m.forward_frames(dev(raw), lengths=frames, **stats)
        assert y.shape == (3, 23, 64)
        tag = "context %s stats %d frames %s" % (fmt, with_stats, frames)
        check_forward(tag, host(y).reshape(-1, 64), exact, emu)
        if frames is None or min(frames) >= 1:                                         # add_context takes T_b >= 1
            rows = fe.add_context(dev(raw), lengths=None if frames is None else list(frames), **stats)
            check_forward(tag + " forward(add_context)", host(m(rows)).reshape(-1, 64), exact, emu)
        y1 = m.forward_frames(dev(raw[1]), lengths=None if frames is None else [frames[1]], **stats)       # [T, D] alone
        assert y1.shape == (23, 64) and torch.equal(bits(y1), bits(y[1])), tag


def test_estimate_mask(mods):
    """dnn_estimate_mask = extract_frame_features -> forward_frames -> clip, for a zero-padded batch"""
    case = dn.small_case()
    m = model(mods, case, "f16", dn.SMALL).eval()
    fe = mods["fe"]
    rng = np.random.default_rng(3)
    noisy = dev((rng.standard_normal((2, 2000)) * 0.1).astype(np.float32))
    lengths = [2000, 1210]
    noisy[1, 1210:] = 0
    mean, std = dn.stats(594, 32)
    mask = mods["training"].dnn_estimate_mask(m, noisy, fe=fe, lengths=lengths, feat_mean=mean, feat_std=std)
    raw = fe.extract_frame_features(noisy, lengths=lengths)
    rows = fe.add_context(raw, mean, std, lengths=[(n - 160) // 80 + 1 for n in lengths])
    ref = m(rows).clamp(0.0, 1.0)
    torch.cuda.synchronize()
    assert mask.shape == (2, 24, 64) and float(mask.min()) >= 0.0 and float(mask.max()) <= 1.0
    exact = dn.forward64(case["Ws"], case["bs"], host(rows).reshape(-1, 594))[0]
    emu = dn.forward64(case["Ws"], case["bs"], host(rows).reshape(-1, 594), fmt=torch.float16)[0]
    check_forward("estimate_mask", host(mask).reshape(-1, 64), exact, emu)
    check_forward("estimate_mask, materialised", host(ref).reshape(-1, 64), exact, emu)


# ---------------------------------------------------------------------------------------------------------------------------
# training: dropout, the node's backward, signs, one optimiser step
# ---------------------------------------------------------------------------------------------------------------------------
def train_forward(mods, case, fmt, dims, k, x=None, need_x=False):
    """the model in train() after torch.manual_seed(k) -> (model, x, y, saved activations as float64, seeds per hidden layer)"""
    m = model(mods, case, fmt, dims).train()
    x = dev(case["x"]) if x is None else x
    x = x.clone().requires_grad_(need_x)
    torch.manual_seed(k)
    y = m(x)
    acts, _, _ = saved(y)
    torch.cuda.synchronize()
    return m, x, y, acts, dn.layer_seeds(dc.drawn_seed(k), len(dims) - 2)


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_dropout(mods, fmt):
    case, dims, p = dn.small_case(), dn.SMALL, dn.P_DROP
    M = dn.SMALL_ROWS
    m, _, y, acts, seeds = train_forward(mods, case, fmt, dims, 11)
    assert m.dropout_rate == p and m.network[2].p == p
    kept32 = np.float64(dc.inv_keep32(p))
    for l in range(3):
        N, K = dims[l + 1], dims[l]
        keep = dc.keep_bits(seeds[l], 0, M * N, p).reshape(M, N)
        h = host(acts[l + 1])[:, :N]
        a = host(acts[l])[:, :K]                            # the operand the device multiplied, exactly
        Wr = dn.rnd(case["Ws"][l], FMTS[fmt])
        z = a @ Wr.T + case["bs"][l]
        tau = K * U32 * (np.abs(a) @ np.abs(Wr).T + np.abs(case["bs"][l]))          # fp32 accumulation, any order
        assert (h[~keep] == 0).all(), l                                               # dropped: exactly 0
        live = keep & (z > tau)
        assert live.sum() > 0.3 * keep.sum() and (h[live] > 0).all(), l
        want = z * kept32
        bound = tau * kept32 + U16[fmt] * np.abs(want) + 2.0 ** -25
        assert (np.abs(h - want)[live] <= bound[live]).all(), (l, float((np.abs(h - want) - bound)[live].max()))
        assert (h[keep & (z < -tau)] == 0).all(), l
        print("dropout %s layer %d: kept %.3f, live %d, max|h - z/(1-p)| / bound %.2f"
              % (fmt, l, keep.mean(), live.sum(), float((np.abs(h - want)[live] / bound[live]).max())))
    _, _, y2, acts2, _ = train_forward(mods, case, fmt, dims, 11)
    assert torch.equal(bits(y), bits(y2)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(acts, acts2))
    _, _, _, acts3, seeds3 = train_forward(mods, case, fmt, dims, 12)
    assert seeds3 != seeds
    assert not torch.equal(acts[1] > 0, acts3[1] > 0)                                 # another seed, another mask


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_node_backward(mods, mode, fmt):
    case, dims = dn.small_case(), dn.SMALL
    p = dn.P_DROP if mode == "train" else 0.0
    t = dn.targets(dn.SMALL_ROWS, 64, dn.GOLDEN_SEED + 2)
    results = []
    for _ in range(2):
        if mode == "train":
            m, x, y, acts, _ = train_forward(mods, case, fmt, dims, 13, need_x=True)
        else:
            m = model(mods, case, fmt, dims).eval()
            x = dev(case["x"]).requires_grad_(True)
            y = m(x)
            acts = saved(y)[0]
        hs = [host(a)[:, :dims[l]] for l, a in enumerate(acts)]
        yd = host(y)
        dy = dn.mse_grad(yd, t)
        for q in list(m.parameters()) + [x]:
            q.grad = None
        y.backward(dev(dy))
        torch.cuda.synchronize()
        results.append([x.grad] + [q.grad for q in m.parameters()])
    for a, b in zip(*results):
        assert torch.equal(bits(a), bits(b))                                           # run to run
    dx, dWs, dbs = dn.backward64(case["Ws"], hs, yd, dy, p=p)
    ex, eWs, ebs = dn.backward64(case["Ws"], hs, yd, dy, p=p, fmt=FMTS[fmt])
    got = results[0]
    named = [("dx", got[0], dx, ex)]
    for l in range(4):
        named += [("dW%d" % l, got[1 + 2 * l], dWs[l], eWs[l]), ("db%d" % l, got[2 + 2 * l], dbs[l], ebs[l])]
    for name, g, exact, emu in named:
        g = host(g)
        assert g.shape == exact.shape and np.isfinite(g).all(), name                  # every element written
        r, re = dn.rel(g, exact), dn.rel(emu, exact)
        print("backward %s %s %s: rel %.3e (emulation %.3e, ratio %.2f)" % (mode, fmt, name, r, re, r / max(re, 1e-300)))
        assert r <= 4.0 * re, (name, r, re)
    if mode == "eval":
        # frozen input: no dx is computed, the parameter gradients are the same bits
        m2 = model(mods, case, fmt, dims).eval().enable_eval_autograd()
        y2 = m2(dev(case["x"]))
        assert y2.requires_grad
        y2.backward(dev(dy))
        torch.cuda.synchronize()
        for a, q in zip(got[1:], m2.parameters()):
            assert torch.equal(bits(a), bits(q.grad))


def test_sign_agreement(mods):
    case, dims, p = dn.default_case(), dn.DEFAULT, dn.P_DROP
    M = case["x"].shape[0]
    _, _, _, acts, seeds = train_forward(mods, case, "f16", dims, 17)
    keeps = [dc.keep_elems(s, 0, M * 1024, p).reshape(M, 1024) for s in seeds]
    _, zs, _ = dn.forward64(case["Ws"], case["bs"], case["x"], keeps=keeps)
    shares = [dn.flip_share(host(acts[l + 1]), zs[l], keeps[l]) for l in range(3)]
    print("sign agreement f16: layers %s overall %.2e" % (["%.2e" % s for s in shares], float(np.mean(shares))))
    assert max(shares) <= 1e-3, shares


def test_one_adam_step(mods):
    """torch.optim.Adam on the ordinary fp32 parameters with MSEMaskLoss as the criterion: they change, and the step is
    reproducible bit for bit"""
    case, dims = dn.small_case(), dn.SMALL
    t = dev(dn.targets(dn.SMALL_ROWS, 64, dn.GOLDEN_SEED + 2))
    ends = []
    for _ in range(2):
        m = model(mods, case, "f16", dims).train()
        crit = mods["training"].MSEMaskLoss()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        torch.manual_seed(19)
        before = [q.detach().clone() for q in m.parameters()]
        opt.zero_grad()
        loss = crit(m(dev(case["x"])), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        for q, b in zip(m.parameters(), before):
            assert q.dtype == torch.float32 and bool(torch.isfinite(q).all()) and not torch.equal(q, b)
        ends.append([q.detach().clone() for q in m.parameters()] + [loss.detach()])
    for a, b in zip(*ends):
        assert torch.equal(bits(a), bits(b))
