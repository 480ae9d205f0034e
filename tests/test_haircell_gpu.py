"""The Meddis hair cell on the device (csrc/haircell.hip through signal_processing.MeddisHairCell) against the float64
restatement of tests/haircell_cases.py, fed the very input the kernel read: what GammatoneFilterbank.filter returned on the
device, [64, 559] and [2, 20, 1153], at scale 1 and at 1e4 (where both clamps act throughout).

  rate      process / process_filterbank: bitwise the restatement (every step is one IEEE double operation in the same order).
  frames    process_to_frames: within 1e-12 relative, elementwise, of the restatement's frame means (the reassociation of a
            160-term fp64 mean of non-negative terms); 0 from T_b on with lengths; an utterance of a padded batch gets the bits
            it gets alone; two runs give the same bits."""
import numpy as np
import pytest
import torch

import gammatone_cases as gc
import haircell_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from sincformer_metacog_speech_enhancement_amd.signal_processing import GammatoneFilterbank, MeddisHairCell
    x64 = GammatoneFilterbank().filter(gc.case_signal("d559").cuda())
    sig = torch.stack([gc.case_signal("c1153"), gc.signal(1153, 331, "noise")]).cuda()
    x20 = GammatoneFilterbank(num_channels=20).filter(sig)
    torch.cuda.synchronize()
    assert x64.shape == (64, 559) and x20.shape == (2, 20, 1153) and x64.dtype == torch.float32
    return {"hc": MeddisHairCell(), "c64": x64, "b20": x20, "ref": {}}


def _case(dev, name, scale):
    """(device input, float64 restatement of the rate on exactly that input)"""
    x = (dev[name] * np.float32(scale)).contiguous()
    key = (name, scale)
    if key not in dev["ref"]:
        dev["ref"][key] = hc.haircell(x.cpu().double())
    return x, dev["ref"][key]


@pytest.mark.parametrize("scale", hc.SCALES)
@pytest.mark.parametrize("name", ["c64", "b20"])
def test_rate_is_bitwise_the_restatement(dev, name, scale):
    x, ref = _case(dev, name, scale)
    got = dev["hc"].process_filterbank(x)
    again = dev["hc"].process_filterbank(x)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and got.shape == x.shape and got.is_cuda
    differ = int((got.cpu() != ref).sum())
    print("ROW | haircell rate %s x%g | %d of %d values differ from the float64 restatement | %d exact zeros" % (
        name, scale, differ, ref.numel(), int((ref == 0).sum())))
    assert torch.equal(got.cpu(), ref) and torch.equal(got, again)
    if scale > 1:
        assert int((ref == 0).sum()) > 100                                  # the clamps acted
    row = x.reshape(-1, x.shape[-1])[3]
    assert torch.equal(dev["hc"].process(row).cpu(), ref.reshape(-1, ref.shape[-1])[3])


@pytest.mark.parametrize("scale", hc.SCALES)
@pytest.mark.parametrize("name", ["c64", "b20"])
def test_frame_means(dev, name, scale):
    x, ref = _case(dev, name, scale)
    want = hc.frames(ref)
    got = dev["hc"].process_to_frames(x)
    again = dev["hc"].process_to_frames(x)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and got.shape == want.shape
    rel = float(((got.cpu() - want).abs() / want.abs().clamp_min(1e-300)).max())
    print("ROW | haircell frames %s x%g | bound %.1e | observed %.2e relative, elementwise" % (name, scale, hc.FRAMES_RTOL, rel))
    assert bool(((got.cpu() - want).abs() <= hc.FRAMES_RTOL * want.abs()).all())
    assert torch.equal(got, again)


def test_other_framings(dev):
    """frame <= hop (a sample lies in at most one frame) and hop < frame < 2 hop"""
    x, ref = _case(dev, "c64", 1e4)
    for frame, hop in ((64, 64), (50, 70), (100, 70)):
        want = hc.frames(ref, frame, hop)
        got = dev["hc"].process_to_frames(x, frame, hop).cpu()
        assert got.shape == want.shape
        assert bool(((got - want).abs() <= hc.FRAMES_RTOL * want.abs()).all()), (frame, hop)


@pytest.mark.parametrize("scale", hc.SCALES)
def test_ragged_batch_is_bitwise_the_single_calls(dev, scale):
    x, _ = _case(dev, "b20", scale)
    lengths = list(hc.RAGGED_LENGTHS)
    got = dev["hc"].process_to_frames(x, lengths=lengths)
    again = dev["hc"].process_to_frames(x, lengths=torch.tensor(lengths))
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    for b, Lb in enumerate(lengths):
        alone = dev["hc"].process_to_frames(x[b, :, :Lb].contiguous())
        Tb = alone.shape[-1]
        assert Tb == (Lb - hc.FRAME) // hc.HOP + 1
        assert torch.equal(got[b, :, :Tb], alone) and bool((got[b, :, Tb:] == 0).all())
