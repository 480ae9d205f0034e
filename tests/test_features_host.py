"""signal_processing/features.py without a GPU: the host-built windows and matrices against the reference's own
(tests/golden/g20_features.npz), the float64 restatement of tests/feature_cases.py against the reference's captured outputs, the
AMS trap, the mutants that the GPU rows' bounds must reject, the argument guards and the launch costs the new wrappers state.

Measured here.  Host operands, in ulp (2^-52) of the array's largest value: mel, bark, equal loudness and AMS triangles 0 (bit for
bit), Hamming(160) and Hamming(128) 0.5, the DCT rows 3.2 (M = 64) and 2.6 (M = 21; scipy takes them through an FFT); the Bark and
mel scale functions 0.  The restatement against the reference, max |diff| / max |ref| per block: RASTA-PLP 5.1e-16, MFCC 1.1e-15,
GFCC 4.9e-11 (the reference filters with fftconvolve, which leaves 1e-16 of the signal's largest value inside the exact zeros; the
cube root lifts that to 1e-11 of the block), context 0, stand-alone vectors 1.0e-15 (GFCC 2.2e-11)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import feature_cases as fc
import helpers as hp
import ops_stub
from sincformer_metacog_speech_enhancement_amd import config, lib, ops
from sincformer_metacog_speech_enhancement_amd.signal_processing import (FeatureExtractor, bark_to_hz, extract_ams, extract_gfcc,
                                                                         extract_mfcc, extract_rasta_plp, hz_to_bark, hz_to_mel,
                                                                         mel_filterbank, mel_to_hz)
from sincformer_metacog_speech_enhancement_amd.signal_processing import features as ft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64, F32 = torch.float64, torch.float32
ULPS = 4.0                                                   # the host operands' bound: a few ulp of float64
REF_TOL = 1e-9                                               # the restatement against the reference (see the docstring: GFCC)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "g20_features.npz"))


def _ulps(a, b):
    assert a.shape == b.shape and a.dtype == np.float64
    return float(np.abs(a - b).max() / (np.abs(b).max() * 2.0 ** -52))


def test_config_values():
    assert (config.AMS_SEGMENTS, config.AMS_OVERLAP, config.AMS_FFT_SIZE, config.AMS_NUM_BANDS) == (128, 64, 256, 15)
    assert (config.MFCC_NUM_COEFF, config.MFCC_FFT_SIZE, config.MFCC_NUM_FILTERS) == (13, 512, 64)
    assert (config.GFCC_NUM_COEFF, config.GFCC_DECIMATE_RATE, config.RASTA_NUM_COEFF, config.CONTEXT_FRAMES) == (13, 100, 13, 5)


def test_host_operands_equal_the_reference(fixture):
    rows = [("hamming160", ft.hamming(160), fixture["hamming160"]), ("hamming128", ft.hamming(128), fixture["hamming128"]),
            ("dct64", ft.dct_rows(13, 64), fixture["dct64"]), ("dct21", ft.dct_rows(13, 21), fixture["dct21"])]
    for fs in (8000, 16000):
        bark, eql = ft.bark_filterbank(fs)
        rows += [("mel.%d" % fs, mel_filterbank(64, 512, fs), fixture["mel.%d" % fs]), ("bark.%d" % fs, bark, fixture["bark.%d" % fs]),
                 ("eql.%d" % fs, eql, fixture["eql.%d" % fs]), ("ams_tri.%d" % fs, ft.ams_filterbank(fs), fixture["ams_tri.%d" % fs])]
    grid = fixture["scales.grid"]
    scales = np.stack([hz_to_bark(grid), bark_to_hz(hz_to_bark(grid)), hz_to_mel(grid), mel_to_hz(hz_to_mel(grid))])
    rows.append(("scales", scales, fixture["scales"]))
    for name, got, ref in rows:
        u = _ulps(got, ref)
        print("HOST | %s %s | %.2f ulp of the largest value" % (name, got.shape, u))
        assert u <= ULPS, (name, u)
    assert fixture["mel.8000"].shape == (64, 257) and fixture["bark.8000"].shape == (21, 129)


def test_the_ams_block_of_the_fixture_is_exactly_zero(fixture):
    """trap 1: inside extract_frame_features the AMS window is 640 samples, 80 after the decimation: shorter than one segment"""
    for name in fc.CASES:
        frames = fixture[name + ".frames"]
        assert frames.shape[1] == 54 and not frames[:, fc.BLOCKS["ams"]].any(), name
        assert frames[:, fc.BLOCKS["mfcc"]].any() and frames[:, fc.BLOCKS["gfcc"]].any() and frames[:, fc.BLOCKS["rasta"]].any()
    assert all(fixture[name + ".ams"].max() > 1.0 for name in fc.AMS_CASES)          # stand-alone, on a longer signal: not zero
    assert not fixture["s401.ams"].any()


@pytest.mark.parametrize("name", list(fc.CASES))
def test_float64_restatement_equals_the_reference(fixture, name):
    ref = torch.from_numpy(fixture[name + ".frames"])
    a = fc.frame_features(name, F64)
    assert a.shape == ref.shape
    worst = {}
    for block, cut in fc.BLOCKS.items():
        worst[block] = float((a[:, cut] - ref[:, cut]).abs().max()) / max(float(ref[:, cut].abs().max()), 1e-300)
    alone = fc.standalone(name, F64)
    for q, v in alone.items():
        r = torch.from_numpy(fixture["%s.%s" % (name, q)])
        worst["alone " + q] = float((v - r).abs().max()) / max(float(r.abs().max()), 1e-300)
    if name in fc.GOLDEN_CONTEXT:
        assert torch.equal(fc.context(ref), torch.from_numpy(fixture[name + ".context"]))
    print("REF | %s | %s" % (name, " | ".join("%s %.1e" % kv for kv in worst.items())))
    assert max(worst.values()) <= REF_TOL, worst


def test_a_one_frame_context_is_eleven_copies(fixture):
    ctx = fixture["s160.context"]
    assert ctx.shape == (1, 594) and np.array_equal(ctx, np.tile(fixture["s160.frames"], (1, 11)))


def _ragged_T():
    return (fc.CASES[fc.RAGGED[0]][2] - fc.FRAME) // fc.HOP + 1


@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_gpu_bounds_reject_the_mutants(mutant):
    """each wrong form against the bound of the GPU row that is meant to catch it (tests/test_features_gpu.py)"""
    if mutant.startswith("pre-emphasis"):
        cut, name, kw = fc.BLOCKS["mfcc"], "s2403", {"mutant": mutant}
    elif mutant.startswith("GFCC"):
        cut, name, kw = fc.BLOCKS["gfcc"], "s2403", {"mutant": mutant}
    elif mutant.startswith("RASTA"):                         # the ragged batch: row 1 after row 0
        cut, name, kw = fc.BLOCKS["rasta"], fc.RAGGED[1], {"state_from": fc.RAGGED[0]}
    elif mutant.startswith("mean over T"):                   # the ragged batch: row 2 has 12 of the batch's 29 frames
        cut, name, kw = fc.BLOCKS["rasta"], fc.RAGGED[2], {"mean_over": _ragged_T()}
    elif mutant.startswith("DCT"):
        cut, name, kw = fc.BLOCKS["mfcc"], "s1153", {"mutant": mutant}
    else:                                                    # the gather is checked exactly: bound 0
        feat = fc.frame_features("s2403", F64)
        good, bad = fc.context(feat), fc.context(feat, mutant=mutant)
        hp.separates("context", mutant, bad, good, good, fc.K)
        assert not torch.equal(fc.context(feat, Tb=12, mutant=mutant), fc.context(feat, Tb=12))
        return
    a64, a32, bad = fc.frame_features(name, F64), fc.frame_features(name, F32), fc.frame_features(name, F64, **kw)
    hp.separates("%s %s" % (name, mutant.split()[0]), mutant, bad[:, cut], a64[:, cut], a32[:, cut], fc.K)
    if mutant.startswith("DCT"):                             # every block that goes through the DCT sees it
        for block in ("rasta", "gfcc"):
            c = fc.BLOCKS[block]
            hp.separates("%s %s" % (name, block), mutant, bad[:, c], a64[:, c], a32[:, c], fc.K)


def test_normalisation_statistics_reach_the_clip():
    mean, std = fc.statistics()
    out = fc.context(fc.frame_features("s2403", F64), mean=mean, std=std)
    assert float(out.abs().max()) == 10.0 and float((out.abs() == 10.0).double().mean()) < 0.5


def test_host_tensors_and_bad_arguments_are_refused():
    fe = FeatureExtractor()
    assert (fe.fs, fe.context, fe.raw_feature_dim, fe.feature_dim, fe.gfb.sample_rate) == (8000, 5, 54, 594, 8000)
    assert FeatureExtractor(16000).gfb.sample_rate == 16000
    x = torch.zeros(400)
    for call in (lambda: fe.extract_frame_features(x), lambda: fe.add_context(torch.zeros(4, 54)), lambda: extract_mfcc(x),
                 lambda: extract_gfcc(x), lambda: extract_rasta_plp(x), lambda: extract_ams(x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError):
        fe.extract_frame_features(np.zeros(400, dtype=np.float32))
    for fs in (11025, 44100, 22050):                          # the GFCC window is not made of whole blocks of the fused kernel
        with pytest.raises(ValueError, match="whole hop-blocks"):
            FeatureExtractor(fs)
    assert ft.gfcc_blocks(8000, fe.gfb, True) == (40, 2, 1, 80) and ft.gfcc_blocks(8000, fe.gfb, False) == (40, 2, 0, 80)
    assert ft.gfcc_blocks(16000, FeatureExtractor(16000).gfb, True) == (80, 1, 0, 160)


def test_entry_points_check_their_arguments_without_a_gpu():
    """argument validation happens before any HIP call"""
    from sincformer_metacog_speech_enhancement_amd import build
    build.build(verbose=False)
    L = lib.load()
    one = ctypes.c_void_p(16)
    cep = lambda *a: L.sfm_cepstral(*a)
    #                in   fb   dct  len   out  B  T   L    fr   hop  mode ld_in im   F    M   NC cmp P  bm ba win  ld_out col
    assert cep(None, one, one, None, one, 1, 4, 400, 160, 80, 0, 772, 257, 257, 64, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -1
    assert cep(one, one, None, None, one, 1, 4, 400, 160, 80, 0, 772, 257, 257, 64, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -1   # NC without dct
    assert cep(one, one, one, None, one, 1, 5, 400, 160, 80, 0, 772, 257, 257, 64, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -2    # T frames do not fit L
    assert cep(one, one, one, None, one, 1, 4, 400, 160, 80, 0, 772, 257, 258, 64, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -2    # F > 257
    assert cep(one, one, one, None, one, 1, 4, 400, 160, 80, 0, 772, 257, 257, 65, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -2    # M > 64
    assert cep(one, one, one, None, one, 1, 4, 400, 160, 80, 0, 772, 257, 257, 64, 13, 1, 0, 1, 0, 1.0, 54, 42, None) == -2    # columns past the row
    assert cep(one, one, one, None, one, 1, 4, 400, 160, 80, 0, 772, 600, 257, 64, 13, 1, 0, 1, 0, 1.0, 54, 28, None) == -2    # im past ld_in
    assert cep(one, None, one, None, one, 1, 4, 400, 160, 80, 2, 0, 0, 64, 64, 13, 2, 8, 2, 1, 80.0, 54, 41, None) == -2       # block 2 n + 2 = 8 >= P
    assert L.sfm_rasta(one, None, one, None, one, 1, 4, 400, 160, 80, 21, 13, 54, 15, None) == -1
    assert L.sfm_rasta(one, one, one, None, one, 1, 4, 400, 160, 80, 65, 13, 54, 15, None) == -2
    assert L.sfm_feature_context(one, one, None, None, one, 1, 4, 4, 1, 1, 54, 5, 10.0, None) == -1                            # mean without std
    assert L.sfm_feature_context(one, None, None, None, one, 1, 4, 4, 1, 1, 53, 5, 10.0, None) == -2                           # odd D
    assert L.sfm_rows_mean(one, None, one, 1, 4, 400, 160, 80, 13, 0, 14, 0, None) == -2


def test_front_end_costs(monkeypatch):
    rec = ops_stub.install(monkeypatch)
    B, T, L = 3, 29, 2403
    spec, out = torch.zeros(B, T, 772), torch.zeros(B, T, 54)
    fr = dict(B=B, T=T, L=L, frame=160, hop=80)
    ops.cepstral(spec[:, :, :514], torch.zeros(64, 257), torch.zeros(13, 64), out, 28, in_mode=ops.CEP_POWER, F=257, im_off=257,
                 compress=ops.CEP_LOG, **fr)
    logb = torch.zeros(B, T, 21)
    ops.cepstral(spec[:, :, 514:], torch.zeros(21, 129), None, logb, 0, in_mode=ops.CEP_POWER, F=129, im_off=129, compress=ops.CEP_LOG, **fr)
    ops.rasta(logb, torch.zeros(21, dtype=torch.float64), torch.zeros(13, 21, dtype=torch.float64), out, 15, L=L, frame=160, hop=80)
    ops.cepstral(torch.zeros(B, 60, 64, 5), None, torch.zeros(13, 64), out, 41, in_mode=ops.CEP_BLOCKS, F=64, compress=ops.CEP_CBRT,
                 bmul=2, badd=1, window=80.0, **fr)
    mean = torch.zeros(594)
    assert ops.feature_context(out, 5, L=T, frame=1, hop=1).shape == (B, T, 594)
    ops.feature_context(out, 5, L=T, frame=1, hop=1, mean=mean, std=mean)
    assert ops.rows_mean(out, 28, 13, L=L, frame=160, hop=80).shape == (B, 13)
    assert rec == [
        ("sfm_cepstral", "cepstral", 3079365.0, 252516.0, "B3 T29 F257 M64 NC13 in0 c1"),
        ("sfm_cepstral", "cepstral", 506862.0, 107928.0, "B3 T29 F129 M21 NC0 in0 c1"),
        ("sfm_rasta", "rasta", 23562.0, 14184.0, "B3 T29 M21 NC13"),
        ("sfm_cepstral", "cepstral", 167040.0, 52396.0, "B3 T29 F64 M64 NC13 in2 c2"),
        ("sfm_feature_context", "feature_context", 0.0, 225504.0, "B3 T29 D54 ctx5 norm0"),
        ("sfm_feature_context", "feature_context", 155034.0, 230256.0, "B3 T29 D54 ctx5 norm1"),
        ("sfm_rows_mean", "rows_mean", 1131.0, 4680.0, "B3 T29 N13"),
    ]
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.cepstral(spec[:, :, :514], torch.zeros(65, 257), None, out, 0, in_mode=ops.CEP_POWER, F=257, im_off=257, compress=0, **fr)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.feature_context(torch.zeros(B, T, 53), 5, L=T, frame=1, hop=1)
