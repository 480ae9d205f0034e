"""The DNN front end on the device (csrc/features.hip through signal_processing.FeatureExtractor, the stand-alone extractors
and training.dnn_frame_pairs) against the float64 restatement of tests/feature_cases.py.

Every numeric row goes through helpers.check_row with k = 16: the device result within 16 x e32 of the float64 restatement, e32 =
the float32 evaluation of the same restatement on the CPU against the float64 one, on the same inputs.
  rasta / mfcc / gfcc   the three live blocks of [T, 54], each a row of its own; the AMS block must be exactly 0.
  silent                the MFCC rows of wholly silent frames against the constant that log(1e-10) gives, within the MFCC bound.
  alone                 extract_mfcc / extract_gfcc / extract_rasta_plp / extract_ams.
  context               the gather exactly (torch.equal against the restatement's gather of the device's own features); the
                        normalisation within e32 (k = 1) of its float64 evaluation on the device's features.
The ragged batch is bitwise the single calls, dnn_frame_pairs bitwise its two halves, two runs give the same bits.
Every row prints `ROW | ...`; profiles/README.md keeps the table."""
import pytest
import torch

import feature_cases as fc
import helpers as hp

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
LIVE = ("rasta", "mfcc", "gfcc")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd import signal_processing as sp, training
    return {"fe": {8000: sp.FeatureExtractor(), 16000: sp.FeatureExtractor(16000)}, "sp": sp, "training": training, "feat": {}}


def _features(dev, name):
    if name not in dev["feat"]:
        fe = dev["fe"][fc.CASES[name][1]]
        dev["feat"][name] = fe.extract_frame_features(fc.case_signal(name).cuda())
        torch.cuda.synchronize()
    return dev["feat"][name]


@pytest.mark.parametrize("name", list(fc.CASES))
def test_frame_features(dev, name):
    got = _features(dev, name).cpu()
    a64, a32 = fc.frame_features(name, F64), fc.frame_features(name, F32)
    assert got.shape == a64.shape and got.dtype == torch.float32 and not got.requires_grad
    assert bool((got[:, fc.BLOCKS["ams"]] == 0).all())
    for block in LIVE:
        cut = fc.BLOCKS[block]
        hp.check_row("%s %s" % (block, name), got[:, cut], a64[:, cut], a32[:, cut], fc.K)
    first, last = fc.silent_frames(name)
    if name in ("s1041", "s1153", "s2403", "k2403"):
        assert last - first >= 2
    if last > first:
        cut = fc.BLOCKS["mfcc"]
        const = fc.silent_mfcc_row()[None, :].expand(last - first, -1)
        assert float((a64[first:last, cut] - const).abs().max()) <= 1e-12          # the restatement's silent rows ARE that constant
        hp.check_row("silent %s" % name, got[first:last, cut], const, a32[first:last, cut], fc.K)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_standalone_extractors(dev, name):
    sp, fs = dev["sp"], fc.CASES[name][1]
    x = fc.case_signal(name).cuda()
    got = {"mfcc": sp.extract_mfcc(x, fs), "gfcc": sp.extract_gfcc(x, fs, gfb=dev["fe"][fs].gfb), "rasta": sp.extract_rasta_plp(x, fs),
           "ams": sp.extract_ams(x, fs)}
    torch.cuda.synchronize()
    a64, a32 = fc.standalone(name, F64), fc.standalone(name, F32)
    for q in ("mfcc", "gfcc", "rasta"):
        assert got[q].shape == (13,) and got[q].dtype == torch.float32
        hp.check_row("alone %s %s" % (q, name), got[q].cpu(), a64[q], a32[q], fc.K)
    assert got["ams"].shape == (15,)
    if name in fc.AMS_CASES:
        hp.check_row("alone ams %s" % name, got["ams"].cpu(), a64["ams"], a32["ams"], fc.K)
    else:
        assert not a64["ams"].any() and bool((got["ams"] == 0).all())         # the decimated signal is shorter than a segment


def _ragged():
    lengths = [fc.CASES[n][2] for n in fc.RAGGED]
    x = torch.zeros(len(lengths), max(lengths))
    for i, n in enumerate(fc.RAGGED):
        x[i, :lengths[i]] = fc.case_signal(n)
    return x, lengths


def test_ragged_batch_rows_equal_the_single_calls_bitwise(dev):
    fe = dev["fe"][8000]
    x, lengths = _ragged()
    batch = fe.extract_frame_features(x.cuda(), lengths=lengths)
    again = fe.extract_frame_features(x.cuda(), lengths=torch.tensor(lengths))
    torch.cuda.synchronize()
    assert batch.shape == (3, 29, 54) and torch.equal(batch, again)               # two runs: the same bits
    for i, n in enumerate(fc.RAGGED):
        single = _features(dev, n)
        Tb = single.shape[0]
        assert torch.equal(batch[i, :Tb], single), n
        assert bool((batch[i, Tb:] == 0).all()), n
    same = fe.extract_frame_features(torch.stack([fc.case_signal("s1153"), fc.case_signal("s1153")]).cuda())
    assert torch.equal(same[0], same[1]) and torch.equal(same[0], _features(dev, "s1153"))       # sample -1 of row 1 reads as 0
    short = fe.extract_frame_features(x.cuda(), lengths=[2403, 100, 1041])        # a short utterance inside a longer buffer
    p = torch.zeros(100)
    p[:] = x[1, :100]
    assert torch.equal(short[1, :1], fe.extract_frame_features(p.cuda())) and bool((short[1, 1:] == 0).all())


@pytest.mark.parametrize("name", ["s160", "s401", "s2403"])
def test_context_is_an_exact_gather(dev, name):
    fe = dev["fe"][8000]
    feat = _features(dev, name)
    got = fe.add_context(feat)
    torch.cuda.synchronize()
    assert got.shape == (feat.shape[0], 594) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), fc.context(feat.cpu()))
    if name == "s160":
        assert torch.equal(got.cpu(), feat.cpu().repeat(1, 11))                    # one frame: 11 copies


def test_context_normalisation_and_ragged_rows(dev):
    fe = dev["fe"][8000]
    mean, std = fc.statistics()
    feat = _features(dev, "s2403").clone()
    feat[3, 30] = float("nan")
    feat[4, 31] = float("inf")
    feat[5, 32] = float("-inf")
    got = fe.add_context(feat, mean.cuda(), std.numpy())
    torch.cuda.synchronize()
    f = feat.cpu()
    r64, r32 = fc.context(f.double(), mean=mean, std=std), fc.context(f, mean=mean, std=std)
    hp.check_row("context normalised s2403", got.cpu(), r64, r32, 1.0)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) == 10.0
    x, lengths = _ragged()
    batch = fe.extract_frame_features(x.cuda(), lengths=lengths)
    frames = [(L - fc.FRAME) // fc.HOP + 1 for L in lengths]
    for stats in ((), (mean.cuda(), std.cuda())):
        ctx = fe.add_context(batch, *stats, lengths=frames)
        assert ctx.shape == (3, 29, 594)
        for i, Tb in enumerate(frames):
            assert torch.equal(ctx[i, :Tb], fe.add_context(batch[i, :Tb].contiguous(), *stats)), i
            assert bool((ctx[i, Tb:] == 0).all())


@pytest.mark.parametrize("mask_type", ["irm", "opt_pcirm"])
def test_dnn_frame_pairs_equal_their_halves_bitwise(dev, mask_type):
    training, fe = dev["training"], dev["fe"][8000]
    x, lengths = _ragged()
    noisy = x.cuda()
    noise = torch.stack([fc.case_signal("s2403").flip(0)] * 3).cuda() * 0.5
    clean = noisy - noise
    mean, std = fc.statistics()
    feats, mask = training.dnn_frame_pairs(clean, noise, noisy, mask_type, fe=fe, lengths=lengths, feat_mean=mean, feat_std=std)
    torch.cuda.synchronize()
    assert feats.shape == (3, 29, 594) and mask.shape == (3, 29, 64)
    frames = [(L - fc.FRAME) // fc.HOP + 1 for L in lengths]
    raw = fe.extract_frame_features(noisy, lengths=lengths)
    assert torch.equal(feats, fe.add_context(raw, mean, std, lengths=frames))
    assert torch.equal(mask, training.gammatone_mask_target(clean, noise, noisy, mask_type, gfb=fe.gfb, lengths=lengths))
    one_f, one_m = training.dnn_frame_pairs(clean[0], noise[0], noisy[0], mask_type, fe=fe)
    assert one_f.shape == (29, 594) and one_m.shape == (29, 64)
    assert torch.equal(one_f, fe.add_context(_features(dev, "s2403")))
