"""Generator of tests/golden/g20_features.npz and tests/golden/g21_haircell.npz.  Runs ONLY where the reference is checked out
(SFM_REFERENCE names its root) and scipy is installed, on the CPU: imports the reference's signal_processing/features.py and
haircell.py - never shipped, never copied - and stores what they return, data only, on the seeded cases of
tests/feature_cases.py and tests/haircell_cases.py.

g20_features.npz
  hamming<n>                   scipy.signal.windows.hamming(n), n = 160 and 128 (float64)
  mel.<fs> / bark.<fs> / eql.<fs>   mel_filterbank(64, 512, fs) [64, 257]; the bark matrix [21, 129] and the equal-loudness
                               vector [21] that extract_rasta_plp builds (captured from inside it), fs = 8000 and 16000
  dct<M>                       the first 13 rows of scipy.fftpack.dct(eye(M), type=2, norm='ortho', axis=0), M = 64 and 21
  ams_tri.<fs>                 the 15 triangles [15, 129] of extract_ams (rebuilt from its outputs on unit spectra: see below)
  scales                       hz_to_bark / bark_to_hz / hz_to_mel / mel_to_hz on a fixed grid
  <case>.frames                FeatureExtractor(fs).extract_frame_features(signal) [T, 54]
  <case>.context               FeatureExtractor(fs).add_context(frames) [T, 594], for GOLDEN_CONTEXT
  <case>.mfcc / .gfcc / .rasta / .ams   the stand-alone extractors on the case signal [13] / [15]
g21_haircell.npz
  q0c0w0.<fs>, dt.<fs>         the steady state and the step of MeddisHairCell(fs), fs = 8000 and 16000
  x.<scale>                    rows haircell_cases.GOLDEN_ROWS of the [64, 559] input, float32, at each scale
  rate.<scale> / frames.<scale>   process_filterbank / process_to_frames of those rows (float64)

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_features.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_features: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)


def haircell():
    import haircell_cases as hc
    from signal_processing.haircell import MeddisHairCell
    out = {}
    for fs in (8000, 16000):
        m = MeddisHairCell(fs)
        out["q0c0w0.%d" % fs] = np.array([m.q0, m.c0, m.w0], dtype=np.float64)
        out["dt.%d" % fs] = np.float64(m.dt)
    m = MeddisHairCell()
    for scale in hc.SCALES:
        x = (hc.inputs("c64")[list(hc.GOLDEN_ROWS)] * np.float32(scale)).numpy()
        assert x.dtype == np.float32
        rate = m.process_filterbank(x.astype(np.float64))
        out["x.%g" % scale], out["rate.%g" % scale] = x, rate
        out["frames.%g" % scale] = m.process_to_frames(x.astype(np.float64))
        print("haircell scale %g: rate %s in [%.3e, %.3e], %d exact zeros" % (scale, rate.shape, rate.min(), rate.max(),
                                                                              int((rate == 0).sum())))
    path = os.path.join(HERE, "g21_haircell.npz")
    np.savez_compressed(path, **out)
    print("g21_haircell %.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1024


class _Recorder:
    """numpy, except that the arrays zeros() and ones() hand out are remembered: the reference builds its bark matrix, its
    equal-loudness vector and its AMS triangles in place inside such arrays, so after a call they hold exactly its values"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(np, name)

    def zeros(self, *a, **kw):
        self.made.append(np.zeros(*a, **kw))
        return self.made[-1]

    def ones(self, *a, **kw):
        self.made.append(np.ones(*a, **kw))
        return self.made[-1]


def features():
    import feature_cases as fc
    from scipy.fftpack import dct
    from scipy.signal.windows import hamming
    import signal_processing.features as rf
    out = {"hamming160": hamming(160), "hamming128": hamming(128)}
    for M in (64, 21):
        out["dct%d" % M] = dct(np.eye(M), type=2, norm="ortho", axis=0)[:13]
    grid = np.array([0.0, 50.0, 440.0, 1000.0, 3999.5, 8000.0])
    out["scales"] = np.stack([rf.hz_to_bark(grid), rf.bark_to_hz(rf.hz_to_bark(grid)), rf.hz_to_mel(grid), rf.mel_to_hz(rf.hz_to_mel(grid))])
    out["scales.grid"] = grid
    probe = fc.case_signal("s2403").numpy().astype(np.float64)
    for fs in (8000, 16000):
        out["mel.%d" % fs] = rf.mel_filterbank(64, 512, fs)
        rec = _Recorder()
        rf.np = rec
        try:
            rf.extract_rasta_plp(probe, fs)
            bark = [a for a in rec.made if a.shape == (21, 129)][0]
            eql = [a for a in rec.made if a.shape == (21,)][0]
            rec.made = []
            rf.extract_ams(probe, fs)
            tri = np.stack([a for a in rec.made if a.shape == (129,)][:15])
        finally:
            rf.np = np
        out["bark.%d" % fs], out["eql.%d" % fs], out["ams_tri.%d" % fs] = bark.copy(), eql.copy(), tri
    for name, (_, fs, L, _, _) in fc.CASES.items():
        x = fc.case_signal(name).numpy().astype(np.float64)
        fe = rf.FeatureExtractor(fs)
        frames = fe.extract_frame_features(x)
        assert frames.shape[1] == 54 and fe.raw_feature_dim == 54 and fe.feature_dim == 594
        assert not frames[:, :15].any(), name                                # trap 1: the AMS block is exactly 0
        out[name + ".frames"] = frames
        if name in fc.GOLDEN_CONTEXT:
            out[name + ".context"] = fe.add_context(frames)
        out[name + ".mfcc"], out[name + ".gfcc"] = rf.extract_mfcc(x, fs), rf.extract_gfcc(x, fs, gfb=fe.gfb)
        out[name + ".rasta"], out[name + ".ams"] = rf.extract_rasta_plp(x, fs), rf.extract_ams(x, fs)
        print("%s fs %d L %d -> %s, stand-alone AMS max %.3e" % (name, fs, L, frames.shape, out[name + ".ams"].max()))
    path = os.path.join(HERE, "g20_features.npz")
    np.savez_compressed(path, **out)
    print("g20_features %.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    which = sys.argv[1:] or ["features", "haircell"]
    if "haircell" in which:
        haircell()
    if "features" in which:
        features()
