"""The ragged EnhancementPath on the host: the length chain, the plan and its tables, the refusals, the new wrappers' contracts.
No GPU: the plan is host arithmetic, the refusals come before any launch, the wrappers run against the stub library."""
import numpy as np
import pytest
import torch

import ops_stub
import ragged_path_cases as rp
from sincformer_metacog_speech_enhancement_amd import functional as Fn, lib, ops
from sincformer_metacog_speech_enhancement_amd.agents.cpea import CorrelationPhaseEstimationAgent
from sincformer_metacog_speech_enhancement_amd.agents.perception import PerceptionAgent
from sincformer_metacog_speech_enhancement_amd.training.conformer_pipeline import EnhancementPath

F16, F32, I32 = torch.float16, torch.float32, torch.int32


# ---------------------------------------------------------------------------
# the length chain
# ---------------------------------------------------------------------------
def test_chain_equals_conv1d_shapes_for_every_length():
    rp.check_chain(Fn.ragged_length_chain)
    rp.check_chain(Fn.ragged_length_chain, lengths=rp.LENGTHS, batch=[4300, 129])       # ... whatever shares the call


def test_frames_equal_the_centred_stft():
    ch = Fn.ragged_length_chain(rp.LENGTHS + [129, 159, 160, 161, 4300])
    assert [int(t) for t in ch["T"]] == [rp.stft_frames(L) for L in rp.LENGTHS + [129, 159, 160, 161, 4300]]


def test_the_chain_constant_is_the_modules_convs():
    pa = PerceptionAgent()
    convs = [b.main[0] for b in pa.conv_blocks] + [pa.downsample[0]]
    assert tuple((c.kernel_size[0], c.stride[0], c.padding[0]) for c in convs) == Fn.PA_CONV_CHAIN == rp.CONVS
    for b in pa.conv_blocks:                                  # the other convs of a block keep or reproduce the row count
        assert (b.main[3].kernel_size[0], b.main[3].stride[0], b.main[3].padding[0]) == (3, 1, 1)
        assert (b.skip[0].kernel_size[0], b.skip[0].stride[0], b.skip[0].padding[0]) == (1, 2, 0)
    L = np.arange(129, 4301)
    assert np.array_equal((L + 2 * 3 - 7) // 2 + 1, (L + 2 * 0 - 1) // 2 + 1)             # skip rows == main rows


@pytest.mark.parametrize("mutant", [rp.mutant_off_by_one, rp.mutant_tpa_from_lmax], ids=["off-by-one", "tpa-from-lmax"])
def test_a_wrong_chain_is_caught(mutant):
    with pytest.raises(AssertionError):
        rp.check_chain(mutant(Fn.ragged_length_chain), lengths=rp.LENGTHS)


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
def test_plan_tables():
    plan = Fn.RaggedPlan(rp.LENGTHS)
    L_ = lib.load()
    for b, L in enumerate(rp.LENGTHS):
        rows = rp.conv_shape_chain(L)
        tin, tout = rows[4], 1 + L // rp.HOP
        fpt = L_.sfm_headpool_frames_per_tile(tin, tout)
        assert fpt > 0 and tuple(plan.headpool[b]) == (tin, tout, fpt, -(-tout // fpt))
        assert int(plan.slots["sinc"][b]) == L_.sfm_sinc_fir16_tiles(L)
        for name, n in zip(("b0", "b1", "b2", "down"), rows[1:]):
            assert int(plan.slots[name][b]) == 2 * -(-n // 128)
    assert plan.max_rows == [4177, 2089, 1045, 523] and (plan.Tpa_max, plan.T_max) == (262, 53)
    assert plan.seg.frame_counts.tolist() == [21, 26, 26, 26, 41, 53, 21] and plan.seg.sum_L == sum(rp.LENGTHS)
    assert plan.tpa_offsets.tolist() == np.concatenate([[0], np.cumsum(plan.Tpa)]).tolist()


def test_the_cached_plan_and_its_tables_are_reused(monkeypatch):
    a = Fn.ragged_plan(rp.LENGTHS)
    assert Fn.ragged_plan(list(rp.LENGTHS)) is a and Fn.ragged_plan(np.asarray(rp.LENGTHS)) is a and Fn.ragged_plan(a) is a
    assert Fn.ragged_plan(rp.LENGTHS[::-1]) is not a
    t = a.tables("cpu")
    def second_upload(x):
        raise AssertionError("the cached tables were built again")
    monkeypatch.setattr(torch, "from_numpy", second_upload)
    assert a.tables("cpu") is t
    monkeypatch.undo()
    for i, r in enumerate(a.rows):
        assert t["rows"][i].dev.tolist() == r.tolist() and t["rows"][i].total == int(r.sum())
    assert t["Tpa"].dev.tolist() == a.Tpa.tolist() and t["T"].dev.tolist() == a.T.tolist()
    assert t["headpool"].tolist() == a.headpool.tolist() and t["tpa_off"].tolist() == a.tpa_offsets.tolist()
    assert {k: v.tolist() for k, v in t["slots"].items()} == {k: v.tolist() for k, v in a.slots.items()}
    assert all(v.dtype is I32 for v in t["slots"].values()) and t["headpool"].dtype is I32
    ft = Fn.frame_table([3, 5, 4], "cpu", 5)
    assert Fn.frame_table((3, 5, 4), "cpu", 5) is ft and ft.total == 12
    with pytest.raises(ValueError):
        Fn.frame_table([3, 6], "cpu", 5)


# ---------------------------------------------------------------------------
# the refusals: loud, before the first launch, with no GPU present
# ---------------------------------------------------------------------------
def _fake_pack(C0=64, K=251, D=256):
    class PW:
        Npad, ksize = 2 * D, 1
    return {"C0": C0, "K": K, "D": D, "zproj": PW(), "blocks": [{"cout": 128}, {"cout": 128}, {"cout": 256}]}


@pytest.fixture
def no_launch(monkeypatch):
    rec = ops_stub.install(monkeypatch)
    yield rec
    assert rec == []


def test_train_mode_and_autograd_are_refused(no_launch):
    wave = torch.zeros(2, 2000)
    path = EnhancementPath()
    with pytest.raises(RuntimeError, match="inference"):
        path.train().forward_ragged(wave, [2000, 1500])
    with pytest.raises(RuntimeError, match="inference"):
        path.eval().forward_ragged(wave.clone().requires_grad_(True), [2000, 1500])
    with pytest.raises(RuntimeError, match="inference"):
        path.train().enhance_batch([np.zeros(2000, np.float32)])
    with pytest.raises(RuntimeError, match="inference"):
        PerceptionAgent().train().forward_channels_last(wave, lengths=[2000, 1500])
    with pytest.raises(RuntimeError, match="inference"):
        CorrelationPhaseEstimationAgent().train()(torch.zeros(2, 26, 256), lengths=[26, 19])
    with pytest.raises(RuntimeError, match="requires grad"):
        Fn.perception_forward(wave.clone().requires_grad_(True), _fake_pack(), latents=False, lengths=[2000, 1500])


def test_memory_and_latents_are_refused(no_launch):
    wave = torch.zeros(2, 2000)
    with pytest.raises(NotImplementedError, match="memory"):
        EnhancementPath(use_memory=True).eval().forward_ragged(wave, [2000, 1500])
    with pytest.raises(NotImplementedError, match="memory"):
        Fn.enhance_path_ragged(wave, [2000, 1500], {"pa": _fake_pack()}, use_memory=True)
    with pytest.raises(NotImplementedError, match="latents"):
        EnhancementPath().eval().forward_ragged(wave, [2000, 1500], want=("mask", "latents"))
    with pytest.raises(NotImplementedError, match="latents"):
        Fn.enhance_path_ragged(wave, [2000, 1500], {"pa": _fake_pack()}, want=("latents",))
    with pytest.raises(NotImplementedError, match="latents"):
        Fn.perception_forward(wave, _fake_pack(), latents=True, lengths=[2000, 1500])


def test_the_unfused_front_end_and_bf16_are_refused(no_launch, monkeypatch):
    wave = torch.zeros(2, 2000)
    packs = {"pa": _fake_pack(), "cpea": {"H": 128, "oc": 64}}
    monkeypatch.setattr(Fn, "PATCH_CONV", False)
    assert not Fn._patch_conv_ok(packs["pa"])
    with pytest.raises(NotImplementedError, match="conv16p"):
        Fn.enhance_path_ragged(wave, [2000, 1500], packs)
    with pytest.raises(NotImplementedError, match="conv16p"):
        Fn.perception_forward(wave, packs["pa"], latents=False, lengths=[2000, 1500])
    monkeypatch.setattr(Fn, "PATCH_CONV", True)
    assert Fn._patch_conv_ok(packs["pa"])
    ops.set_compute_dtype(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="fp16"):
        Fn.enhance_path_ragged(wave, [2000, 1500], packs)
    ops.set_precision_policy({"pa": torch.bfloat16, "front": F16, "block": F16, "attn": F16, "tail": F16})
    with pytest.raises(NotImplementedError, match="fp16"):
        Fn.perception_forward(wave, packs["pa"], latents=False, lengths=[2000, 1500])


def test_another_lstm_is_refused(no_launch):
    wave = torch.zeros(2, 2000)
    with pytest.raises(NotImplementedError, match="128"):
        Fn.enhance_path_ragged(wave, [2000, 1500], {"pa": _fake_pack(), "cpea": {"H": 64, "oc": 64}})
    z16 = torch.zeros(52, 256, dtype=F16)
    with pytest.raises(NotImplementedError, match="128"):
        Fn.cpea_forward(z16, {"H": 64}, 2, 26, lengths=[26, 19])
    with pytest.raises(NotImplementedError, match="128"):
        CorrelationPhaseEstimationAgent(hidden_size=64).eval()(torch.zeros(2, 26, 256), lengths=[26, 19])
    ops.set_lstm_w16(False)
    try:
        with pytest.raises(NotImplementedError, match="lstm_w16"):
            Fn.cpea_forward(z16, {"H": 128}, 2, 26, lengths=[26, 19])
        with pytest.raises(NotImplementedError, match="lstm_w16"):
            Fn.enhance_path_ragged(wave, [2000, 1500], {"pa": _fake_pack(), "cpea": {"H": 128, "oc": 64}})
    finally:
        ops.set_lstm_w16(True)


def test_a_short_utterance_is_refused(no_launch):
    assert Fn.RAGGED_MIN_SAMPLES == rp.N_FFT // 2 + 1 == 129
    Fn.RaggedPlan([129, 4000])
    with pytest.raises(ValueError, match="utterance 1 has 128 samples"):
        Fn.RaggedPlan([4000, 128])
    with pytest.raises(ValueError, match="128 samples"):
        EnhancementPath().eval().forward_ragged(torch.zeros(2, 4000), [4000, 128])
    with pytest.raises(ValueError, match="128 samples"):
        EnhancementPath().eval().enhance_batch([np.zeros(4000, np.float32), np.zeros(128, np.float32)])
    with pytest.raises(ValueError):
        Fn.RaggedPlan([])


# ---------------------------------------------------------------------------
# the new wrappers: one valid call reaches the launcher with the header's argument count and a stated cost; a defect is refused
# ---------------------------------------------------------------------------
def _pw(N, K, ksize, cin):
    return ops.PackedWeight(torch.zeros(N, K, dtype=F16), torch.zeros(N), N, K, ksize, cin, False)


def _i32(*v):
    return torch.tensor(v, dtype=I32)


def _wrapper_calls():
    B, Lin, cin, N = 2, 100, 64, 128
    x = torch.zeros(B, Lin, cin, dtype=F16)
    sc = torch.zeros(B, cin)
    return {
        "sinc_fir16_varlen": (ops.sinc_fir16_varlen, (torch.zeros(B, 300), _i32(300, 200), torch.zeros(64, 251),
                                                      torch.zeros(B, 300, 64, dtype=F16), 64, 251, 500), {}, 1),
        "conv16p_varlen": (ops.conv16p_varlen, (x, sc, sc, _pw(N, 7 * cin, 7, cin), torch.zeros(B, 50, N, dtype=F16), _i32(100, 61),
                                                _i32(50, 31)), dict(B=B, Lin=Lin, stride=2, pad=3, n_out=81), 5),
        "gn_finalize_varlen": (ops.gn_finalize_varlen, (torch.zeros(B, 4, 8, 2), torch.ones(64), torch.zeros(64), _i32(50, 31),
                                                        _i32(2, 2), B, 4, 8, 64), {}, 3),
        "gn_apply_varlen": (ops.gn_apply_varlen, (torch.zeros(B, 50, 256, dtype=F16), torch.zeros(B, 256), torch.zeros(B, 256),
                                                  torch.zeros(B, 50, 256, dtype=F16), _i32(50, 31), B, 50, 256, 81), {}, 4),
        "headpool_varlen": (ops.headpool_varlen, (torch.zeros(B, 50, 256, dtype=F16), _pw(512, 256, 1, 256),
                                                  torch.zeros(B, 12, 512, dtype=F16), torch.zeros(B, 1, 32, 2),
                                                  torch.tensor([[50, 12, 12, 1], [31, 8, 8, 1]], dtype=I32), B, 50, 12, 1, 81, 20), {}, 4),
        "bilstm_layer_rows16_varlen": (ops.bilstm_layer_rows16_varlen, (torch.zeros(B, 12, 2, 512), torch.zeros(2, 512, 128),
                                                                        _i32(12, 8), B, 12, 128, 20), {}, 2),
        "rows_gather32": (ops.rows_gather32, (torch.zeros(B * 12, 768, dtype=F16), torch.zeros(20, 1088, dtype=F16), _i32(12, 8),
                                              _i32(0, 12, 20), B, 12, 768, 20), {}, 2),
    }


@pytest.mark.parametrize("name", sorted(_wrapper_calls()))
def test_a_ragged_wrapper_launches_once_and_refuses_a_wrong_table(monkeypatch, name):
    ops.set_compute_dtype(F16)
    rec = ops_stub.install(monkeypatch)
    fn, args, kw, table_at = _wrapper_calls()[name]
    fn(*args, **kw)
    assert len(rec) == 1 and rec[0][0] == "sfm_" + name and rec[0][3] > 0, rec       # one launch, a stated byte count
    del rec[:]
    bad = list(args)
    bad[table_at] = bad[table_at].to(torch.int64)                                      # the length table in the wrong format
    with pytest.raises(RuntimeError, match="unsupported shape"):
        fn(*bad, **kw)
    assert rec == []


def test_ragged_costs_count_the_valid_rows(monkeypatch):
    ops.set_compute_dtype(F16)
    rec = ops_stub.install(monkeypatch)
    fn, args, kw, _ = _wrapper_calls()["conv16p_varlen"]
    fn(*args, **kw)
    fn, args, kw, _ = _wrapper_calls()["bilstm_layer_rows16_varlen"]
    fn(*args, **kw)
    assert rec == [("sfm_conv16p_varlen", "conv16p", 2.0 * 81 * 128 * 448, 162 * 64 * 2.0 + 81 * 128 * 2 + 128 * 448 * 2.0,
                    "Lout81 Cin64 N128 k7 s2 in1 varlen"),
                   ("sfm_bilstm_layer_rows16_varlen", "bilstm_layer", 2.0 * 20 * 2 * 4 * 128 * 128, 20 * 8 * 128 * 4 + 24 * 256 * 2, None)]


def test_the_header_declares_the_ragged_entry_points():
    for name in ("sfm_sinc_fir16_varlen", "sfm_conv16p_varlen", "sfm_gn_finalize_varlen", "sfm_gn_apply_varlen", "sfm_headpool_varlen",
                 "sfm_bilstm_layer_rows16_varlen", "sfm_rows_gather32"):
        assert name in lib.ABI, name
        assert hasattr(lib.load(), name), name
