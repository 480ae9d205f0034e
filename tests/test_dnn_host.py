"""SpeechEnhancementDNN without a GPU: the float64 restatement of tests/dnn_cases.py against the reference's recorded results
(tests/golden/g22_dnn.npz), the module's host side (keys, shapes, `or` defaults, load_rbm_weights), the argument guards of the two
entry points through the built library, the launch costs the wrappers state, and a proof on the CPU that the bounds of
tests/test_dnn_gpu.py - 4 x the error of the operand-rounding emulation - catch plausible wrong kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dnn_cases as dn
import ops_stub

HERE = os.path.dirname(os.path.abspath(__file__))
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "g22_dnn.npz"))


@pytest.fixture(scope="module")
def pkg():
    from sincformer_metacog_speech_enhancement_amd import config, models, ops
    return {"config": config, "models": models, "ops": ops}


def golden_params(golden):
    Ws = [golden["state.network.%d.weight" % (3 * l)] for l in range(4)]
    bs = [golden["state.network.%d.bias" % (3 * l)] for l in range(4)]
    return Ws, bs


# ---- the restatement against the reference's recorded results ----
def test_restatement_forward_matches_the_fixture(golden):
    Ws, bs = golden_params(golden)
    gen = dn.params(dn.SMALL, dn.GOLDEN_SEED)
    for a, b in zip(Ws + bs, gen[0] + gen[1]):
        assert np.array_equal(a, b)                             # the fixture's state is the seeded one
    y, _, _ = dn.forward64(Ws, bs, dn.inputs(dn.SMALL_ROWS, 594, dn.GOLDEN_SEED + 1))
    assert golden["y"].shape == (37, 64)
    assert np.abs(y - golden["y"]).max() < 2e-6                 # the reference computed in float32
    assert dn.small_case()["y"] is not None and np.array_equal(dn.small_case()["y"], y)


def test_restatement_backward_matches_the_fixture(golden):
    Ws, bs = golden_params(golden)
    y, _, hs = dn.forward64(Ws, bs, dn.inputs(dn.SMALL_ROWS, 594, dn.GOLDEN_SEED + 1))
    dy = dn.mse_grad(y, dn.targets(dn.SMALL_ROWS, 64, dn.GOLDEN_SEED + 2))
    _, dWs, dbs = dn.backward64(Ws, hs, y, dy)
    assert np.array_equal(golden["grad_cols"], dn.GRAD_COLS)
    for l in range(4):
        dW = dWs[l][:, dn.GRAD_COLS] if l == 0 else dWs[l]
        assert dn.rel(golden["grad.network.%d.weight" % (3 * l)], dW) < 1e-5, l
        assert dn.rel(golden["grad.network.%d.bias" % (3 * l)], dbs[l]) < 1e-5, l


# ---- the module's host side ----
def test_default_model_keys_shapes_and_count(golden, pkg):
    m = pkg["models"].SpeechEnhancementDNN()
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in golden["default.keys"]]
    assert list(sd) == ["network.%d.%s" % (3 * l, n) for l in range(4) for n in ("weight", "bias")]
    for v, shape in zip(sd.values(), golden["default.shapes"]):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]]
    assert m.count_parameters() == int(golden["default.count"]) == 2774080
    c = pkg["models"].create_dnn(594)
    assert (c.input_dim, c.hidden_dim, c.output_dim, c.num_hidden_layers, c.dropout_rate) == (594, 1024, 64, 3, 0.2)
    assert pkg["models"].create_dnn(162, 32).network[9].weight.shape == (32, 1024)
    assert [type(x).__name__ for x in m.network] == ["Linear", "ReLU", "Dropout"] * 3 + ["Linear", "Sigmoid"]
    assert len(m.get_layer_params()) == 4 and m.get_layer_params()[0][0] is m.network[0].weight


def test_config_values_are_the_references(pkg):
    cfg = pkg["config"]
    assert (cfg.DNN_HIDDEN_LAYERS, cfg.DNN_HIDDEN_UNITS, cfg.DNN_DROPOUT) == (3, 1024, 0.2)
    assert (cfg.DNN_LEARNING_RATE, cfg.DNN_EPOCHS, cfg.DNN_BATCH_SIZE) == (0.001, 50, 256)


def test_constructor_keeps_the_or_defaults(golden, pkg):
    z = pkg["models"].SpeechEnhancementDNN(0, 0, 0, 0, 0)
    got = [z.input_dim, z.hidden_dim, z.output_dim, z.num_hidden_layers, z.dropout_rate]
    assert got == [float(v) for v in golden["or_defaults"]] == [594, 1024, 64, 3, 0.2]
    assert z.network[2].p == 0.2


def test_load_rbm_weights(golden, pkg):
    Ws, bs = golden_params(golden)
    for as_tensor in (False, True):
        m = pkg["models"].SpeechEnhancementDNN(594, 64, 64, 3)
        m.load_state_dict(dn.state_dict(Ws, bs))
        tuples = dn.rbm_tuples(dn.SMALL, dn.GOLDEN_SEED + 3)
        if as_tensor:
            tuples = [tuple(torch.from_numpy(a) for a in t) for t in tuples]
        m.load_rbm_weights(tuples)
        for k, v in m.state_dict().items():
            want = golden["rbm." + k]
            assert np.array_equal(v.numpy() if v.dim() == 1 else v.numpy()[::4, ::4], want), k
        assert np.array_equal(m.state_dict()["network.9.weight"].numpy(), Ws[3])         # the output layer is never set
        assert np.array_equal(m.state_dict()["network.0.weight"].numpy(), tuples_w(tuples[0]))


def tuples_w(t):
    w = t[0].numpy() if torch.is_tensor(t[0]) else t[0]
    return w.T.astype(np.float32)


def test_a_host_tensor_is_refused(pkg):
    m = pkg["models"].SpeechEnhancementDNN(594, 64, 64, 3).eval()
    with pytest.raises(RuntimeError, match="CPU"):
        m(torch.zeros(3, 594))
    with pytest.raises(RuntimeError, match="CPU"):
        m.forward_frames(torch.zeros(2, 5, 54))


# ---- argument guards through the built library ----
@pytest.fixture(scope="module")
def L():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def test_dnn_layer_guards_without_a_gpu(L):
    """a null pointer or a bad code gives -1 and a bad shape -2, before any HIP call: every call below is refused, none can reach
    a launch"""
    one = ctypes.c_void_p(16)

    def call(A=one, frames=None, mean=None, std=None, W=one, bias=one, out=one, mode=0, M=4, N=64, K=64, lda=64, T=0, D=0, ctx=0,
             Kpad=64, Npad=64, ldo=64, of32=0, act=1, p=0.0, dt=1):
        return L.sfm_dnn_layer(A, frames, mean, std, W, bias, out, mode, M, N, K, lda, T, D, ctx, Kpad, Npad, ldo, of32, act, p, 0, dt, None)
    assert call(A=None) == -1 and call(W=None) == -1 and call(out=None) == -1
    assert call(dt=7) == -1 and call(mode=3) == -1 and call(act=3) == -1 and call(of32=2) == -1
    assert call(p=1.0) == -1 and call(p=0.2, act=2) == -1           # dropout goes with the ReLU
    assert call(mode=2, mean=one, T=2, D=8, K=8, M=4) == -1          # mean and std go together
    assert call(mode=0, frames=one) == -1                            # the context's operands in another mode
    assert call(A=ctypes.c_void_p(8)) == -1                          # rows16: 16-byte aligned rows
    assert call(M=0) == -2 and call(N=0) == -2 and call(K=0) == -2
    assert call(Kpad=96) == -2 and call(K=65) == -2 and call(Npad=32) == -2 and call(Npad=96) == -2 and call(ldo=63) == -2
    assert call(lda=60) == -2 and call(K=60, lda=60) == -2           # rows16: lda a multiple of 8 that holds round_up(K, 8)
    assert call(mode=1, K=594, Kpad=640, lda=593) == -2              # rows32: lda >= K
    assert call(mode=2, T=3, D=54, ctx=5, K=594, Kpad=640, M=7) == -2        # M is B T
    assert call(mode=2, T=3, D=54, ctx=5, K=590, Kpad=640, M=6) == -2        # K is D (2 ctx + 1)
    assert call(mode=2, T=2, D=6, ctx=0, K=6, M=4) == -2 and call(mode=2, T=2, D=9, ctx=0, K=9, M=4) == -2      # D even and >= 8
    assert call(mode=2, T=2, D=8, ctx=0, K=8, M=4, A=ctypes.c_void_p(4)) == -1                               # read in pairs
    assert call(mode=2, T=3, D=54, ctx=65, K=54 * 131, Kpad=7104, M=6) == -2
    assert call(mode=2, T=1, D=410, ctx=5, K=4510, Kpad=4544, M=2, mean=one, std=one) == -2   # statistics beyond the LDS budget


def test_dnn_act_bwd_guards_without_a_gpu(L):
    one = ctypes.c_void_p(16)

    def call(dy=one, f32=1, ldy=64, saved=one, lds=64, dz=one, ldz=64, M=4, N=64, act=1, p=0.0, dt=1):
        return L.sfm_dnn_act_bwd(dy, f32, ldy, saved, lds, dz, ldz, M, N, act, p, dt, None)
    assert call(dy=None) == -1 and call(dz=None) == -1 and call(saved=None) == -1
    assert call(dt=5) == -1 and call(act=3) == -1 and call(f32=2) == -1 and call(p=1.0) == -1 and call(p=0.2, act=2) == -1
    assert call(dz=ctypes.c_void_p(8)) == -1
    assert call(M=0) == -2 and call(N=0) == -2 and call(ldy=63) == -2 and call(lds=63) == -2 and call(ldz=63) == -2 and call(ldz=68) == -2
    assert call(N=60, ldz=60) == -2


# ---- the launch costs the wrappers state ----
@pytest.fixture
def launches(monkeypatch, pkg):
    rec = ops_stub.install(monkeypatch)
    pkg["ops"].set_compute_dtype(F16)
    return rec


def test_dnn_launch_costs(launches, pkg):
    ops = pkg["ops"]
    M = 200
    first = ops.PackedWeight(torch.zeros(1024, 640, dtype=F16), torch.zeros(1024), 1024, 594, 1, 640)
    hidden = ops.PackedWeight(torch.zeros(1024, 1024, dtype=F16), torch.zeros(1024), 1024, 1024, 1, 1024)
    last = ops.PackedWeight(torch.zeros(64, 1024, dtype=F16), torch.zeros(64), 64, 1024, 1, 1024)
    h = ops.dnn_layer(torch.zeros(M, 594), first, act="relu")
    assert h.shape == (M, 1024) and h.dtype == F16
    ops.dnn_layer(h, hidden, act="relu", p_drop=0.2, seed=3)
    y = ops.dnn_layer(h, last, act="sigmoid", out_dtype=F32)
    assert y.shape == (M, 64) and y.dtype == F32
    ops.dnn_layer(torch.zeros(4, 50, 54), first, act="relu", context=5, frames=torch.zeros(4, dtype=torch.int32),
                  mean=torch.zeros(594), std=torch.ones(594))
    dz = ops.dnn_act_bwd(torch.zeros(M, 64), y, "sigmoid", 64)
    assert dz.shape == (M, 64) and dz.dtype == F16
    ops.dnn_act_bwd(torch.zeros(M, 1024, dtype=F16), h, "relu", 1024, p_drop=0.2)
    assert launches == [
        ("sfm_dnn_layer", "dnn_layer", 2.0 * 200 * 1024 * 594, 200 * 594 * 4 + 1024 * 640 * 2 + 1024 * 4 + 200 * 1024 * 2, "M200 N1024 K594 a1 act1 o2"),
        ("sfm_dnn_layer", "dnn_layer", 2.0 * 200 * 1024 * 1024, 200 * 1024 * 2 + 1024 * 1024 * 2 + 1024 * 4 + 200 * 1024 * 2,
         "M200 N1024 K1024 a0 act1 o2 drop"),
        ("sfm_dnn_layer", "dnn_layer", 2.0 * 200 * 64 * 1024, 200 * 1024 * 2 + 64 * 1024 * 2 + 64 * 4 + 200 * 64 * 4, "M200 N64 K1024 a0 act2 o4"),
        # the context mode reads the raw rows once: 54 columns per row, not 594
        ("sfm_dnn_layer", "dnn_layer", 2.0 * 200 * 1024 * 594, 200 * 54 * 4 + 594 * 8 + 4 * 4 + 1024 * 640 * 2 + 1024 * 4 + 200 * 1024 * 2,
         "M200 N1024 K594 a2 act1 o2"),
        ("sfm_dnn_act_bwd", "dnn_act_bwd", 2.0 * 200 * 64, 200 * 64 * 8 + 200 * 64 * 2, "M200 N64 act2"),
        ("sfm_dnn_act_bwd", "dnn_act_bwd", 2.0 * 200 * 1024, 200 * 1024 * 4 + 200 * 1024 * 2, "M200 N1024 act1"),
    ]


def test_dnn_layer_wrapper_refuses_what_the_kernel_would(launches, pkg):
    ops = pkg["ops"]
    first = ops.PackedWeight(torch.zeros(1024, 640, dtype=F16), torch.zeros(1024), 1024, 594, 1, 640)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.dnn_layer(torch.zeros(8, 600), first)                                   # fp32 rows are [M, K]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.dnn_layer(torch.zeros(8, 594, dtype=F16), first)                        # 16-bit rows hold round_up(K, 8) columns
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.dnn_layer(torch.zeros(2, 4, 54), first, context=4)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.dnn_layer(torch.zeros(2, 4, 54), first, context=5, frames=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="compute format"):
        ops.dnn_layer(torch.zeros(8, 594), ops.PackedWeight(torch.zeros(64, 640, dtype=BF16), torch.zeros(64), 64, 594, 1, 640))
    assert launches == []


# ---- the GPU tests' bounds catch wrong kernels (all on the CPU, float64) ----
FMTS = (F16, BF16)


@pytest.mark.parametrize("fmt", FMTS)
def test_forward_bound_catches_mutants(fmt):
    """bound = 4 x (RMS, max) error of the emulation; a mutant of the exact restatement - no rounding at all - must miss it"""
    c = dn.small_case()
    ye, _, _ = dn.emulation(c, fmt)
    rms_b, max_b = (4.0 * e for e in dn.err(ye, c["y"]))
    for mutant in ("no_bias", "k_tail_zero"):
        ym, _, _ = dn.forward64(c["Ws"], c["bs"], c["x"], mutant=mutant)
        r, m = dn.err(ym, c["y"])
        assert r > rms_b and m > max_b, (mutant, r, rms_b, m, max_b)
    # dropout: the check of the first hidden layer, h = keep z / (1 - p) within tau = 4 x the emulation's largest error there
    keeps = dn.keep_masks(5, dn.SMALL_ROWS, dn.SMALL[1:-1], dn.P_DROP)
    _, _, hs = dn.forward64(c["Ws"], c["bs"], c["x"], keeps=keeps)
    _, _, he = dn.forward64(c["Ws"], c["bs"], c["x"], keeps=keeps, fmt=fmt)
    tau = 4.0 * np.abs(he[1] - hs[1]).max()
    _, _, hm = dn.forward64(c["Ws"], c["bs"], c["x"], keeps=keeps, mutant="no_drop_scale")
    assert np.abs(hm[1] - hs[1]).max() > tau


@pytest.mark.parametrize("fmt", FMTS)
def test_context_bound_catches_mutants(fmt):
    """the context mode is held to the forward bound through the small model: each wrong gather / order must miss it"""
    c = dn.small_case()
    raw, mean, std = dn.context_case()
    frames = dn.CTX_FRAMES
    for st in ((None, None), (mean, std)):
        if st[0] is None:
            r0 = np.where(np.isfinite(raw), raw, 0.0).astype(np.float32)          # without statistics a nan stays a nan: finite cells
        else:
            r0 = raw
        x = dn.context64(r0, frames, mean=st[0], std=st[1]).reshape(-1, 594)
        y, _, _ = dn.forward64(c["Ws"], c["bs"], x)
        ye, _, _ = dn.forward64(c["Ws"], c["bs"], x, fmt=fmt)
        rms_b, max_b = (4.0 * e for e in dn.err(ye, y))
        for mutant in dn.CTX_MUTANTS:
            if mutant == "clip_first" and st[0] is None:
                continue
            xm = dn.context64(r0, frames, mean=st[0], std=st[1], mutant=mutant).reshape(-1, 594)
            ym, _, _ = dn.forward64(c["Ws"], c["bs"], xm)
            r, m = dn.err(ym, y)
            assert r > rms_b and m > max_b, (mutant, st[0] is None, r, rms_b, m, max_b)


@pytest.mark.parametrize("fmt", FMTS)
def test_backward_bound_catches_mutants(fmt):
    """gradients from the same active-and-kept masks: bound = 4 x the emulation's relative RMSE, per gradient"""
    c = dn.small_case()
    keeps = dn.keep_masks(5, dn.SMALL_ROWS, dn.SMALL[1:-1], dn.P_DROP)
    y, _, hs = dn.forward64(c["Ws"], c["bs"], c["x"], keeps=keeps, fmt=fmt)          # the forward the device runs
    dy = dn.mse_grad(y, dn.targets(dn.SMALL_ROWS, 64, dn.GOLDEN_SEED + 2))
    dx, dWs, dbs = dn.backward64(c["Ws"], hs, y, dy, p=dn.P_DROP)
    ex, eWs, ebs = dn.backward64(c["Ws"], hs, y, dy, p=dn.P_DROP, fmt=fmt)
    for mutant in dn.BWD_MUTANTS:
        mx, mWs, mbs = dn.backward64(c["Ws"], hs, y, dy, p=dn.P_DROP, mutant=mutant)
        first = 0 if mutant == "no_drop_scale" else 3                 # the dropout scale enters below the last hidden layer
        for l in range(0, first + 1) if mutant == "no_drop_scale" else range(4):
            assert dn.rel(mWs[l], dWs[l]) > 4.0 * dn.rel(eWs[l], dWs[l]), (mutant, l)
            assert dn.rel(mbs[l], dbs[l]) > 4.0 * dn.rel(ebs[l], dbs[l]), (mutant, l)
        assert dn.rel(mx, dx) > 4.0 * dn.rel(ex, dx), mutant


def test_emulation_sign_share_stays_under_the_cap():
    """the GPU test caps the share of hidden units whose sign differs from float64's at 1e-3; the emulation alone must stay well
    under it (2.5e-4) on the case that test uses (203 x 1024 units per layer), overall and in the worst layer"""
    for c in (dn.default_case(),):
        for fmt in (F16,):
            _, _, he = dn.emulation(c, fmt)
            shares = [dn.flip_share(he[l + 1], c["zs"][l]) for l in range(3)]
            total = float(np.mean(shares))
            print("emulation sign share %s: layers %s overall %.2e" % (fmt, ["%.2e" % s for s in shares], total))
            assert max(shares) < 2.5e-4 and total < 2.5e-4, shares
