"""Training on packed rows, the part that needs no GPU: the refusals of the public interface (before any launch), the span
table of the packed depthwise weight gradient, the ABI, and the references of tests/packed_train_cases.py themselves (they
reduce to the dense restatements on equal lengths, and the wrong variants they carry miss the GPU tests' bounds)."""
import ctypes

import numpy as np
import pytest
import torch

import dropout_cases as dc
import helpers as hp
import ops_stub
import packed_train_cases as pc
import test_abi


@pytest.fixture()
def pkg():
    from sincformer_metacog_speech_enhancement_amd import build, lib, ops

    class NS:
        pass
    build.build(verbose=False)
    ns = NS()
    ns.ops, ns.lib = ops, lib
    return ns


def _enhancer(pkg, monkeypatch, **kw):
    """a SpeechEnhancer on the CPU whose device check is off: every launch it would enqueue lands in the stub's record"""
    from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import SpeechEnhancer
    from sincformer_metacog_speech_enhancement_amd._hostmod import HipModule
    rec = ops_stub.install(monkeypatch)
    monkeypatch.setattr(HipModule, "_require_device", lambda self, *t: None)
    row = dict(n_freq=129, d_model=128, num_blocks=1, num_heads=2, d_ff=256, kernel_size=31, dropout=0.1)
    row.update(kw)
    return SpeechEnhancer(**row), rec


# ---- the three refusals, each before the first launch ---------------------------------------------------------------------------
def test_head_dim_other_than_64_is_refused_before_any_launch(pkg, monkeypatch):
    m, rec = _enhancer(pkg, monkeypatch, d_model=64, num_heads=2)          # head_dim 32
    x = torch.zeros(5, 129)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        m.forward_packed_train(x, x, [2, 3])
    with pytest.raises(NotImplementedError, match="head_dim"):
        m.blocks[0].train().forward_packed(torch.zeros(5, 64), [2, 3])
    assert rec == []


def test_unsupported_depthwise_kernel_size_is_the_existing_refusal(pkg, monkeypatch):
    m, rec = _enhancer(pkg, monkeypatch, kernel_size=15)
    x = torch.zeros(5, 129)
    rm = m.blocks[0].conv.batch_norm.running_mean.clone()
    with pytest.raises(NotImplementedError, match="depthwise kernel_size 15 is not supported"):
        m.forward_packed_train(x, x, [2, 3])
    with pytest.raises(NotImplementedError, match="depthwise kernel_size 15 is not supported"):
        m.blocks[0].train().forward_packed(torch.zeros(5, 128), [2, 3])
    assert rec == [] and torch.equal(rm, m.blocks[0].conv.batch_norm.running_mean)
    assert int(m.blocks[0].conv.batch_norm.num_batches_tracked) == 0


def test_spectra_that_are_not_sum_T_rows_are_refused(pkg, monkeypatch):
    m, rec = _enhancer(pkg, monkeypatch)
    for rows, cols in ((4, 129), (6, 129), (5, 128)):
        x = torch.zeros(rows, cols)
        with pytest.raises(RuntimeError, match=r"expected \[5, 129\]"):
            m.forward_packed_train(x, x, [2, 3])
    with pytest.raises(RuntimeError, match=r"expected \[5, 129\]"):
        m.forward_packed_train(torch.zeros(5, 129), torch.zeros(4, 129), [2, 3])
    with pytest.raises(RuntimeError, match="expected"):
        m.blocks[0].train().forward_packed(torch.zeros(4, 128), [2, 3])
    assert rec == []


def test_forward_packed_still_refuses_train_mode(pkg, monkeypatch):
    m, rec = _enhancer(pkg, monkeypatch)
    x = torch.zeros(5, 129)
    m.train()
    with pytest.raises(RuntimeError, match="inference path"):
        m.forward_packed(x, x, [2, 3])
    m.eval()
    with pytest.raises(RuntimeError, match="inference path"):
        m.forward_packed(x.clone().requires_grad_(True), x, [2, 3])
    assert rec == []


def test_the_node_refuses_rows_that_are_not_the_pack(pkg, monkeypatch):
    """train.block_train_forward itself (the door of anyone who builds the node by hand) checks head_dim, kernel size and
    the row count before its first launch"""
    from sincformer_metacog_speech_enhancement_amd import functional as Fn, train
    rec = ops_stub.install(monkeypatch)
    seg = Fn.PackedSegments([2, 3])
    P = {"conv.depthwise.weight": torch.zeros(256, 1, 31)}
    with pytest.raises(RuntimeError, match="4 rows, expected sum_T = 5"):
        train.block_train_forward(torch.zeros(4, 256), P, None, None, 4, 0.0, 0, seg=seg)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        train.block_train_forward(torch.zeros(5, 256), P, None, None, 8, 0.0, 0, seg=seg)
    with pytest.raises(NotImplementedError, match="head_dim"):
        train.block_train_forward(torch.zeros(5, 256), P, None, None, 3, 0.0, 0, seg=seg)
    assert rec == []


# ---- the span table -------------------------------------------------------------------------------------------------------------
LENGTH_SETS = [pc.CONV_LENGTHS, pc.ATTN_RAGGED, [130, 130, 130], [1], [1, 1, 1], [801] * 64, [512] * 64, [33, 64, 65],
               list(range(201, 802, 7)), [40000, 1, 77]]


@pytest.mark.parametrize("lengths", LENGTH_SETS, ids=lambda l: "n%d-sum%d" % (len(l), sum(l)))
def test_spans_cover_every_frame_once_and_stay_inside_an_utterance(pkg, lengths):
    sp = pkg.ops.dwconv_wgrad_spans(lengths)
    assert sp.dtype == np.int32 and sp.ndim == 2 and sp.shape[1] == 3 and sp.flags["C_CONTIGUOUS"]
    seen = [np.zeros(T, dtype=np.int64) for T in lengths]
    for u, t0, n in sp.tolist():
        assert 0 <= u < len(lengths) and n >= 1 and 0 <= t0 and t0 + n <= lengths[u], (u, t0, n)      # inside ONE utterance
        seen[u][t0:t0 + n] += 1
    assert all((s == 1).all() for s in seen)                                                         # every frame exactly once
    assert (np.diff(sp[:, 0]) >= 0).all()                                                            # utterance order: a fixed fold
    assert len(lengths) <= sp.shape[0] <= pkg.ops.WGRAD_PARTIALS + len(lengths)
    # no span longer than the cut: WGRAD_MIN_SPAN frames, or sum_T / WGRAD_PARTIALS where that is more
    assert int(sp[:, 2].max()) <= max(pkg.ops.WGRAD_MIN_SPAN, -(-sum(lengths) // pkg.ops.WGRAD_PARTIALS))


def test_spans_of_equal_lengths_are_the_dense_launcher_cut(pkg):
    """on B x T the table has the dense launcher's partial count (its scratch size says it: a host function)"""
    L = pkg.lib.load()
    for B, T in ((64, 512), (3, 130), (2, 801), (64, 801), (1, 1)):
        dense = int(L.sfm_dwconv_wgrad_scratch_floats(B, T, 256, 31)) // (32 * 256)
        assert pkg.ops.dwconv_wgrad_spans([T] * B).shape[0] == dense, (B, T)
    with pytest.raises(ValueError):
        pkg.ops.dwconv_wgrad_spans([])
    with pytest.raises(ValueError):
        pkg.ops.dwconv_wgrad_spans([3, 0])


def test_tables_carry_the_spans_and_are_uploaded_once(pkg):
    from sincformer_metacog_speech_enhancement_amd import functional as Fn
    seg = Fn.packed_frames(pc.CONV_LENGTHS)
    assert Fn.packed_frames(list(pc.CONV_LENGTHS)) is seg and Fn.packed_frames(seg) is seg
    tb = seg.tables("cpu", 4)
    assert seg.tables("cpu", 4) is tb and seg.tables("cpu") is tb
    assert tb["wgrad_spans"].dtype == torch.int32
    assert np.array_equal(tb["wgrad_spans"].numpy(), pkg.ops.dwconv_wgrad_spans(pc.CONV_LENGTHS))
    assert np.array_equal(tb["conv_tiles"].numpy(), pkg.ops.dwconv_tiles(pc.CONV_LENGTHS))
    assert tb["frame_off"].tolist() == pc.offsets(pc.CONV_LENGTHS).tolist() and tb["samp_off"] is None
    # one flat upload: the three tables are views of one storage
    assert tb["wgrad_spans"].untyped_storage().data_ptr() == tb["frame_off"].untyped_storage().data_ptr()
    seg2 = Fn.PackedSegments([3, 4], [700, 900])
    assert seg2.tables("cpu")["samp_off"].tolist() == [0, 700, 1600]


# ---- the ABI --------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("sfm_attention_fwd_train_varlen", "sfm_attention_bwd_varlen", "sfm_dwconv_wgrad_varlen",
               "sfm_dwconv_wgrad_varlen_scratch_floats")


def test_the_abi_sets_are_still_equal(pkg):
    decls = test_abi._header_decls()
    assert set(decls) == set(pkg.lib.SIGNATURES)
    raw = ctypes.CDLL(pkg.lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in decls and hasattr(raw, name), name
        assert pkg.lib.SIGNATURES[name] == decls[name][1]
        assert pkg.lib.ABI[name][0] is ctypes.c_int                 # statuses (and a count that fits an int)


def test_the_new_launchers_refuse_without_a_gpu(pkg):
    """argument validation happens before any HIP call"""
    L = pkg.lib.load()
    one = ctypes.c_void_p(16)
    fwd = lambda hd=64, n_items=8, p=0.0, lse=one: L.sfm_attention_fwd_train_varlen(
        one, one, lse, one, one, n_items, 2, 100, 150, 4, hd, 768, 256, 256, 512, -1.0, p, 1, 7, None)
    assert fwd() == -1                                              # control: every shape check passed, the dtype is refused
    assert fwd(lse=None) == -1
    assert fwd(hd=32) == -2 and fwd(n_items=7) == -2 and fwd(n_items=9) == -2 and fwd(p=1.0) == -2
    bwd = lambda hd=64, n_items=8, dt=7: L.sfm_attention_bwd_varlen(
        one, one, one, one, one, one, one, one, n_items, 2, 100, 150, 4, hd, 768, 256, 256, 512, 0.0, 1, dt, None)
    assert bwd() == -1 and bwd(hd=16) == -2 and bwd(n_items=7) == -2
    wg = lambda n=4, C=256, KS=31, sum_T=150: L.sfm_dwconv_wgrad_varlen(one, one, one, one, one, one, one, n, 2, sum_T, C, KS, 7, None)
    assert wg() == -1 and wg(KS=15) == -2 and wg(C=255) == -2 and wg(n=1) == -2 and wg(n=70000, sum_T=80000) == -2
    assert L.sfm_dwconv_wgrad_varlen_scratch_floats(5, 256, 31) == 5 * 32 * 256
    assert L.sfm_dwconv_wgrad_varlen_scratch_floats(0, 256, 31) == -2
    assert L.sfm_dwconv_wgrad_varlen_scratch_floats(65535, 4096, 31) == -2         # past 2^31 - 1 floats


def test_wrappers_refuse_with_the_one_refusal_and_state_their_cost(pkg, monkeypatch):
    ops = pkg.ops
    rec = ops_stub.install(monkeypatch)
    ops.set_compute_dtype(torch.float16)
    lengths = [5, 130]
    n, T2 = 135, 5 * 5 + 130 * 130
    off = torch.tensor([0, 5, 135], dtype=torch.int32)
    items = torch.from_numpy(ops.attention_items(lengths, pc.H))
    spans = torch.from_numpy(ops.dwconv_wgrad_spans(lengths))
    qkv = torch.zeros(n, 3 * pc.D, dtype=torch.float16)
    O, lse = ops.attention_train_varlen(qkv, off, items, 2, 130, n, pc.H, 64, sum_T2=T2)
    assert O.shape == (n, pc.D) and lse.shape == (pc.H, n) and lse.dtype == torch.float32
    dqkv = ops.attention_bwd_varlen(qkv, O, O, lse, off, items, 2, 130, n, pc.H, 64, sum_T2=T2)
    assert dqkv.shape == qkv.shape
    dw, db = ops.dwconv_wgrad_varlen(O, torch.zeros(n, pc.D), off, spans, 2, n, pc.D, 31)
    assert dw.shape == (pc.D, 31) and db.shape == (pc.D,)
    assert [r[0] for r in rec] == ["sfm_attention_fwd_train_varlen", "sfm_attention_bwd_varlen", "sfm_dwconv_wgrad_varlen"]
    assert rec[0][2] == 4.0 * pc.H * 64 * T2 and rec[1][2] == 10.0 * pc.H * 64 * T2              # FLOPs from sum T_u^2
    assert rec[2][2] == 2.0 * n * pc.D * 32
    del rec[:]
    bad = [lambda: ops.attention_train_varlen(qkv.float(), off, items, 2, 130, n, pc.H, 64),
           lambda: ops.attention_train_varlen(qkv, off, items, 2, 130, n, 8, 32),                # head_dim 32
           lambda: ops.attention_train_varlen(qkv, off[:2], items, 2, 130, n, pc.H, 64),
           lambda: ops.attention_train_varlen(qkv[:-1], off, items, 2, 130, n, pc.H, 64),
           lambda: ops.attention_train_varlen(qkv, off, items, 2, 130, n, pc.H, 64, lse=torch.zeros(pc.H * n - 1)),
           lambda: ops.attention_bwd_varlen(qkv, O, O[:, :128], lse, off, items, 2, 130, n, pc.H, 64),
           lambda: ops.attention_bwd_varlen(qkv, O, O, lse.double(), off, items, 2, 130, n, pc.H, 64),
           lambda: ops.attention_bwd_varlen(qkv, O, O, lse, off, items.long(), 2, 130, n, pc.H, 64),
           lambda: ops.dwconv_wgrad_varlen(O, torch.zeros(n, pc.D), off, spans, 2, n, pc.D, 15),
           lambda: ops.dwconv_wgrad_varlen(O, torch.zeros(n, pc.D, dtype=torch.float16), off, spans, 2, n, pc.D, 31),
           lambda: ops.dwconv_wgrad_varlen(O, torch.zeros(n, pc.D), off, spans[:1], 2, n, pc.D, 31),
           lambda: ops.dwconv_wgrad_varlen(O, torch.zeros(n, pc.D), off, spans, 2, n, pc.D, 31, dw=torch.zeros(pc.D, 7))]
    for call in bad:
        with pytest.raises(RuntimeError, match=r"failed: unsupported shape \(-2\)"):
            call()
    assert rec == []
    ops.reset_precision()


# ---- the references themselves --------------------------------------------------------------------------------------------------
def test_packed_keep_is_the_dense_replica_on_equal_lengths_and_not_on_ragged_ones():
    T, p = 130, 0.1
    dense = hp.keep_mask(pc.SEED, 3, pc.H, T, p)
    packed = pc.packed_keep(pc.SEED, [T] * 3, pc.H, p)
    assert all(torch.equal(packed[u][0], dense[u]) for u in range(3))
    # the index is unique across a ragged pack: no two probability rows share a hash row
    off = pc.offsets(pc.ATTN_RAGGED)
    rows = np.concatenate([(pc.H * off[u] + h * T_ + np.arange(T_)) for u, T_ in enumerate(pc.ATTN_RAGGED) for h in range(pc.H)])
    assert len(set(rows.tolist())) == rows.size == pc.H * sum(pc.ATTN_RAGGED)
    wrong = pc.packed_keep(pc.SEED, pc.ATTN_RAGGED, pc.H, p, "dense")
    right = pc.packed_keep(pc.SEED, pc.ATTN_RAGGED, pc.H, p)
    assert torch.equal(wrong[0], right[0]) and not any(torch.equal(a, b) for a, b in zip(wrong[2:], right[2:]))


@pytest.mark.parametrize("dt", pc.DTYPES, ids=["f16", "bf16"])
def test_attention_mutants_miss_the_bound(dt):
    """keys of the neighbouring utterance included (p 0) and the dense dropout row index (p 0.1) move O by >= 5 x its bound"""
    ref = pc.attn_case("ragged", dt, 0.0)
    wrong = pc.attn_case("ragged", dt, 0.0, "neighbour keys")
    moved = max(hp.maxerr(w[0], r[0]) for w, r in zip(wrong, ref))
    pc.separates_abs("attention O", "keys of the neighbouring utterance included", moved, 8 * pc.EPS[dt])
    moved = max(hp.maxerr(w[1], r[1]) for w, r in zip(wrong, ref))
    pc.separates_abs("attention LSE", "keys of the neighbouring utterance included", moved, pc.LSE_TOL[dt])
    ref, wrong = pc.attn_case("ragged", dt, 0.1), pc.attn_case("ragged", dt, 0.1, "dense index")
    moved = max(hp.maxerr(w[0], r[0]) for w, r in zip(wrong, ref))
    pc.separates_abs("attention O p 0.1", "dense row index for dropout on a ragged pack", moved, 8 * pc.EPS[dt])
    g = [(hp.maxerr(w[2], r[2]), pc.attn_tols(dt, r[2])[2]) for w, r in zip(wrong[1:], ref[1:])]
    pc.separates_abs("attention dqkv p 0.1", "dense row index for dropout on a ragged pack", *max(g, key=lambda t: t[0] / t[1]))


@pytest.mark.parametrize("KS,C", pc.WGRAD_ROWS)
def test_the_weight_gradient_reference_and_its_mutant(KS, C):
    dt = torch.float16
    c = pc.wgrad_case(KS, C, dt)
    # the sum over utterances is autograd of the packed conv
    w = (hp.arr("pw_w", (C, KS), 5) / KS).double().requires_grad_(True)
    b = hp.arr("pw_b", (C,), 6).double().requires_grad_(True)
    y = pc.dwconv_packed64(c["x"].double(), w, b, pc.CONV_LENGTHS)
    y.backward(c["dy"].double())
    assert hp.figs(c["ref64"][0], w.grad)[1] < 1e-12 and hp.figs(c["ref64"][1], b.grad)[1] < 1e-12
    hp.separates("packed dwconv_wgrad KS%d C%d" % (KS, C), "the conv window crossing an utterance boundary", c["wrong64"][0],
                 c["ref64"][0], c["ref32"][0], hp.K_SUM, c["dw_bound"])


def test_packed_block64_is_block64_on_equal_lengths():
    """the packed restatement on [130, 130, 130] is dropout_cases.block64 on [3, 130, D], batch statistics and masks included"""
    lengths, p, base = [130, 130, 130], 0.1, 12345
    sd, x, _ = pc.block_inputs("equal")
    sd64 = {k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()}
    x64 = x.double()
    for masks_p, masks_d in ((None, None), (pc.packed_masks(base, lengths, pc.D, pc.H, pc.FF, p),
                                            dc.block_masks(base, 3, 130, pc.D, pc.H, pc.FF, p))):
        st_p, st_d = {}, {}
        yp = pc.packed_block64(x64, sd64, lengths, pc.H, False, masks_p, st_p)
        yd = dc.block64(x64.reshape(3, 130, pc.D), sd64, pc.H, masks_d, stats=st_d).reshape(-1, pc.D)
        assert hp.figs(yp, yd)[1] < 1e-11
        assert hp.figs(st_p["mean"], st_d["mean"])[1] < 1e-11 and hp.figs(st_p["var"], st_d["var"])[1] < 1e-11
        assert st_p["n"] == st_d["n"] == 390
    # and the BatchNorm statistics are helpers.bn_stats64's over the valid rows
    ye = pc.packed_block64(x64, sd64, lengths, pc.H, True)
    assert hp.figs(ye, yp)[0] > 1e-3                                # (eval mode is another function: the running statistics moved)
