"""Packed (variable-length) inference, the part that needs no GPU: the host helper that lays a list of signals out, the work
tables of the packed kernels, the argument guards of the five new entry points, and - in the style of test_host_logic.py's
mutant checks - proof that the GPU tests of tests/test_ragged_gpu.py can fail: plausible wrong packed forwards, restated with
the oracle's own functions, move EVERY utterance of the test's length set by at least 5 x the bound it is tested with."""
import ctypes

import numpy as np
import pytest
import torch

import ragged_cases as rc
from helpers import rmse
from sincformer_metacog_speech_enhancement_amd import functional as Fn, ops

# the widest mask bound of the path test (bf16; mixed and fp16 are held to 1e-3) and the STFT kernel's bound
MASK_BOUND = 2e-3
STFT_BOUND = 2e-5


# ---------------------------------------------------------------------------
# packed_segments
# ---------------------------------------------------------------------------
def test_packed_segments_lays_the_length_set_out():
    (seg,) = Fn.packed_segments(rc.LENGTHS)
    assert seg.B == 7 and (seg.start, seg.stop) == (0, 7)
    assert seg.frame_counts.tolist() == rc.FRAMES == [26, 16, 6, 40, 2, 66, 131]
    assert seg.frame_offsets.tolist() == rc.FRAME_OFFSETS
    assert seg.sample_offsets.tolist() == [0, 2000, 3237, 3637, 6757, 6886, 12089, 22489]
    assert (seg.max_T, seg.sum_T, seg.sum_L) == (131, 287, 22489)
    assert seg.sum_T2 == float(sum(t * t for t in rc.FRAMES))


def test_packed_segments_names_the_signal_the_dense_stft_would_refuse():
    with pytest.raises(ValueError, match=r"signal 2 .*L=128"):
        Fn.packed_segments([2000, 129, 128, 400])
    Fn.packed_segments([129])                                   # the shortest admissible signal
    with pytest.raises(ValueError):
        Fn.packed_segments([2000], max_frames=0)
    assert Fn.packed_segments([]) == []


def test_packed_segments_splits_greedily_in_the_given_order():
    passes = Fn.packed_segments(rc.LENGTHS, max_frames=60)
    assert [(p.start, p.stop) for p in passes] == [(0, 3), (3, 5), (5, 6), (6, 7)]      # 26+16+6 | 40+2 | 66 alone | 131 alone
    assert [p.frame_counts.tolist() for p in passes] == [[26, 16, 6], [40, 2], [66], [131]]
    assert all(p.sum_T <= 60 or p.B == 1 for p in passes)
    assert passes[1].frame_offsets.tolist() == [0, 40, 42] and passes[1].sample_offsets.tolist() == [0, 3120, 3249]
    assert [(p.start, p.stop) for p in Fn.packed_segments(rc.LENGTHS, max_frames=48)] == [(0, 3), (3, 5), (5, 6), (6, 7)]
    assert [(p.start, p.stop) for p in Fn.packed_segments(rc.LENGTHS, max_frames=47)] == [(0, 2), (2, 4), (4, 5), (5, 6), (6, 7)]
    assert len(Fn.packed_segments(rc.LENGTHS, max_frames=287)) == 1
    assert len(Fn.packed_segments(rc.LENGTHS, max_frames=1)) == 7


def test_segments_from_frame_counts_alone_and_their_guards():
    seg = Fn.PackedSegments([3, 1, 200])
    assert seg.frame_offsets.tolist() == [0, 3, 4, 204] and seg.sample_offsets is None and seg.max_T == 200
    for bad in ([], [3, 0, 2], [-1]):
        with pytest.raises(ValueError):
            Fn.PackedSegments(bad)


# ---------------------------------------------------------------------------
# work tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 4, 8])
def test_attention_items_hold_every_existing_tile_once_longest_first(H):
    rng = np.random.RandomState(5)
    for T in (rc.FRAMES, [1], [128, 129, 1, 1100, 2], rng.randint(100, 701, 300).tolist()):
        it = ops.attention_items(T, H)
        assert it.dtype == np.int32 and it.shape[1] == 4 and it.flags["C_CONTIGUOUS"]
        want = {(u, h, q) for u, t in enumerate(T) for h in range(H) for q in range(-(-t // 128))}
        got = [tuple(r) for r in it[:, :3].tolist()]
        assert len(got) == len(want) and set(got) == want               # nothing masked, nothing missing, nothing twice
        # longest key range first, up to the dealing within a run of 64: the key ranges of successive runs do not increase
        keys = np.asarray(T)[it[:, 0]]
        runs = [keys[i:i + 64] for i in range(0, len(keys), 64)]
        assert all(a.min() >= b.max() for a, b in zip(runs, runs[1:]))
        # workgroups are dealt round-robin over 8 XCDs: the tiles of one (utterance, head) sit on one XCD when they fit a run
        if len(got) >= 64:
            pos = {g: i for i, g in enumerate(got)}
            same = sum(1 for (u, h, q) in got if q > 0 and pos[(u, h, q - 1)] // 64 == pos[(u, h, q)] // 64
                       and pos[(u, h, q - 1)] % 8 == pos[(u, h, q)] % 8)
            later = sum(1 for (u, h, q) in got if q > 0)
            assert same >= 0.6 * later, (same, later)


def test_dwconv_tiles_hold_every_tile_once():
    for T in (rc.FRAMES, [1], [64, 65, 1, 1100]):
        tl = ops.dwconv_tiles(T)
        want = [(u, j) for u, t in enumerate(T) for j in range(-(-t // 64))]
        assert tl.dtype == np.int32 and [tuple(r) for r in tl.tolist()] == want


# ---------------------------------------------------------------------------
# argument guards of the five entry points (validation happens before any HIP call)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib.load()


one = ctypes.c_void_p(16)
BAD_DT = 7            # an invalid dtype, checked after the shapes: a control passes every shape check and is refused for it (-1)


def test_framed_gemm_varlen_guards(L):
    f = L.sfm_framed_gemm_f32_varlen
    ok = (2, 42, 80, 80, 160, 160, 258, 320, 129, 129, 1, 1, 1)
    assert f(one, one, one, one, one, one, *ok, BAD_DT, None) == -1                                   # control
    for nulls in ((None, one, one, one, one), (one, None, one, one, one), (one, one, None, one, one), (one, one, one, None, one),
                  (one, one, one, one, None)):
        sig, wt, out, so, fo = nulls
        assert f(sig, wt, out, one, so, fo, *ok, 0, None) == -1
    shape = lambda **kw: f(one, one, one, one, one, one, *[kw.get(k, v) for k, v in zip(
        ("B", "sum_T", "hop", "padl", "K", "Kpad", "N", "Npad", "nsplit", "ldm", "ldn", "mode", "out_f32"), ok)], BAD_DT, None)
    assert shape() == -1
    assert shape(B=0) == -2 and shape(sum_T=0) == -2 and shape(hop=0) == -2
    assert shape(Kpad=168) == -2 and shape(Npad=300) == -2 and shape(K=200) == -2 and shape(N=400) == -2
    g = L.sfm_framed_gemm_split16_varlen
    ok16 = (2, 42, 80, 80, 160, 160, 256, 256, 129, 1, 129, 1)
    for i in range(7):
        if i == 4:
            continue                                                                                      # out2 is optional
        ptrs = [one] * 7
        ptrs[i] = None
        assert g(*ptrs, *ok16, None) == -1
    bad = lambda idx, val: g(*[one] * 7, *[val if j == idx else v for j, v in enumerate(ok16)], None)
    assert bad(0, 0) == -2 and bad(1, 0) == -2 and bad(2, 0) == -2 and bad(5, 168) == -2 and bad(7, 300) == -2 and bad(4, 200) == -2


def test_attention_varlen_guards(L):
    f = L.sfm_attention_fwd_varlen

    def call(qkv=one, out=one, fo=one, items=one, n_items=8, B=2, max_T=100, sum_T=150, H=4, hd=64, ldqkv=768, ldo=256, dt=BAD_DT,
             odt=0):
        return f(qkv, out, fo, items, n_items, B, max_T, sum_T, H, hd, ldqkv, ldo, H * hd, 2 * H * hd, -1.0, dt, odt, None)
    assert call() == -1                                                                              # control: shapes accepted
    assert call(qkv=None, dt=0) == -1 and call(out=None, dt=0) == -1 and call(fo=None, dt=0) == -1
    assert call(items=None, dt=0) == -1                                     # head_dim 64 needs the item table
    assert call(B=0) == -2 and call(max_T=0) == -2 and call(sum_T=99) == -2 and call(H=0) == -2
    assert call(hd=0, ldqkv=768) == -2 and call(hd=257, H=1, ldqkv=771, ldo=257) == -2
    assert call(ldqkv=192) == -2 and call(ldo=128) == -2                   # rows narrower than H * hd
    assert call(n_items=7, dt=0) == -2 and call(n_items=9, dt=0) == -2     # 2 x 4 (utterance, head) pairs of one tile each
    assert call(hd=16, ldqkv=192, ldo=64, items=None) == -1                # control: the generic kernel needs no table
    assert call(hd=16, ldqkv=192, ldo=64, items=None, dt=0, odt=1) == -2   # ... and writes the operands' format only


def test_dwconv_varlen_guards(L):
    f = L.sfm_dwconv_folded_varlen

    def call(x=one, w=one, sc=one, sh=one, out=one, fo=one, tiles=one, n_tiles=3, B=2, max_T=100, sum_T=150, C=256, KS=31, dt=BAD_DT):
        return f(x, w, sc, sh, out, fo, tiles, n_tiles, B, max_T, sum_T, C, KS, 1, 0, dt, None)
    assert call() == -1 and call(C=192, KS=15) == -1 and call(C=64, KS=7) == -1                     # controls
    for k in ("x", "w", "sc", "sh", "out", "fo"):
        assert call(**{k: None, "dt": 0}) == -1
    assert call(tiles=None, dt=0) == -1 and call(tiles=None, C=192, KS=15) == -1                     # generic kernel: no table
    assert call(B=0) == -2 and call(max_T=0) == -2 and call(sum_T=99) == -2
    assert call(C=0) == -2 and call(KS=8) == -2 and call(KS=0) == -2 and call(C=192, KS=14) == -2
    assert call(n_tiles=1, dt=0) == -2 and call(n_tiles=5, dt=0) == -2     # 2 utterances of at most 2 tiles each


def test_istft_ola_varlen_guards(L):
    f = L.sfm_istft_ola_varlen
    ok = (2, 3000, 256, 80, 160, 160)
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        assert f(*ptrs, *ok, None) == -1
    bad = lambda idx, val: f(*[one] * 5, *[val if j == idx else v for j, v in enumerate(ok)], None)
    assert bad(0, 0) == -2 and bad(1, 0) == -2 and bad(3, 0) == -2 and bad(4, 0) == -2 and bad(4, 257) == -2 and bad(5, 159) == -2


def test_header_binding_and_library_agree_on_the_new_entry_points(L):
    import test_abi
    from sincformer_metacog_speech_enhancement_amd import lib
    decls = test_abi._header_decls()
    names = ("sfm_framed_gemm_f32_varlen", "sfm_framed_gemm_split16_varlen", "sfm_attention_fwd_varlen", "sfm_dwconv_folded_varlen",
             "sfm_istft_ola_varlen")
    raw = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert decls[n][1] == lib.SIGNATURES[n] and decls[n][0] is getattr(L, n).restype and hasattr(raw, n), n


# ---------------------------------------------------------------------------
# the GPU tests can fail: wrong packed forwards move every utterance by >= 5 x the bound
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    sigs, sd = rc.waves(), rc.enhancer_state()
    return sigs, sd, rc.oracle_alone(sd, sigs)


def _per_utt(mask_packed):
    return mask_packed.split(rc.FRAMES, dim=0)


def test_the_restated_packed_forward_is_the_oracle_on_every_utterance_alone(case):
    """the restatement the mutants are made from, with attention and convolution kept inside each utterance, reproduces the
    reference (so what the mutants change is the only difference)"""
    sigs, sd, ref = case
    nr, ni = torch.cat([r[0] for r in ref]), torch.cat([r[1] for r in ref])
    mm = rc.packed_forward(sd, nr, ni, rc.FRAMES)
    for i, m in enumerate(_per_utt(mm)):
        assert rmse(m, ref[i][4]) < 1e-6, i
    assert 0.4 < float(mm.mean()) < 0.6 and float(mm.std()) > 0.15         # the de-saturated, hard regime


@pytest.mark.parametrize("mutant", ["attention over the whole concatenation", "depthwise convolution over the whole concatenation"])
def test_mixing_utterances_in_attention_or_convolution_is_caught_on_every_utterance(case, mutant):
    sigs, sd, ref = case
    nr, ni = torch.cat([r[0] for r in ref]), torch.cat([r[1] for r in ref])
    kw = dict(attention="all") if mutant.startswith("attention") else dict(conv="all")
    mm = rc.packed_forward(sd, nr, ni, rc.FRAMES, **kw)
    for i, m in enumerate(_per_utt(mm)):
        r = rmse(m, ref[i][4])
        print("MUTANT | %s | utterance %d (T %d) | mask RMSE %.2e = %.0f x the bound" % (mutant, i, rc.FRAMES[i], r, r / MASK_BOUND))
        assert r >= 5 * MASK_BOUND, (mutant, i, r)


def test_zero_padding_to_a_rectangle_is_caught_on_every_shorter_utterance(case):
    sigs, sd, ref = case
    longest = int(np.argmax(rc.LENGTHS))
    for i, m in enumerate(rc.zero_padded_masks(sd, sigs)):
        r = rmse(m, ref[i][4])
        print("MUTANT | zero-padded rectangular batch | utterance %d (T %d) | mask RMSE %.2e" % (i, rc.FRAMES[i], r))
        if i == longest:
            assert r < 1e-5                                                # no padding: the same computation
        else:
            assert r >= 5 * MASK_BOUND, (i, r)


def test_framing_that_runs_into_the_next_utterance_is_caught_on_the_last_frame_of_each(case):
    """exactly one frame per utterance differs, the last - so the kernel test looks at that frame of every utterance on its own"""
    sigs, sd, ref = case
    for i, (re, im) in enumerate(rc.stft_reading_the_neighbour(sigs)):
        got, want = torch.cat([re, im], -1), torch.cat([ref[i][0], ref[i][1]], -1)
        d = (got - want).abs().amax(dim=1)
        rms = float(want.pow(2).mean().sqrt())
        print("MUTANT | framing reads the neighbour | utterance %d | last frame max|err| %.2e (%.2e of the rms), others %.2e" % (
            i, float(d[-1]), float(d[-1]) / rms, float(d[:-1].max())))
        assert float(d[:-1].max()) <= 1e-6 and float(d[-1]) >= 5 * STFT_BOUND, (i, d)
        # pooled over a long utterance the same error hides: its share of the rms of all frames falls with 1 / sqrt(T)
    pooled = rmse(torch.cat([torch.cat(p, -1) for p in rc.stft_reading_the_neighbour(sigs)]),
                  torch.cat([torch.cat([r[0], r[1]], -1) for r in ref]))
    print("pooled rmse of the same mutant over all 287 frames: %.2e" % pooled)
