"""Generator of tests/golden/g21_intelligibility.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root),
on the CPU: imports the reference's evaluation/csii.py and evaluation/ncm.py - never shipped, never copied - and stores what they
return on the seeded cases of tests/intelligibility_cases.py.

  csii.<case> / msc.<case>     compute_csii and _magnitude_squared_coherence of every CSII case (float64, [129])
  csii.ident.<case>            compute_csii(clean, clean)
  csii.len.<fs>                compute_csii at the lengths CSII_GOLDEN_LENGTHS[fs] (property 1 below)
  sii.<fs>                     _speech_importance_function(129, fs, 256) at 8, 16 and 22.05 kHz
  ncm.<case> / ncc.<case>      compute_ncm and the per-channel _normalized_covariance of every NCM case
  chw.<bank>                   the channel weights compute_ncm applies: its value when _normalized_covariance answers 1 for one
                               channel and 0 for the others
  hilbert.h<L> / hilbert.y<L>  scipy.signal.hilbert(.).imag of the unit impulse and of intelligibility_cases.hilbert_rows(L), L = 64, 65

It asserts, again, the two properties the device code rests on:
  1. compute_csii does not depend on its amplitude regions: with frame = int(0.016 fs) it is 0.0 below one frame and otherwise
     clip(sum(w * msc), 0, 1) of ONE coherence estimate over the whole signal, for num_levels 1, 3 and 5;
  2. hilbert(x).imag is the circular convolution with h = imag(ifft(H)) (intelligibility_cases.hilbert64), at L = 64, 65, 401,
     1237 and 2000;
and that no case sits where an fp32 bound means nothing: every sqrt(var_x var_y) and every Pxx Pyy is exactly 0 or above 1e-6.

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_intelligibility.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_intelligibility: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import intelligibility_cases as ic  # noqa: E402


def main():
    from scipy.signal import hilbert
    from evaluation import csii as rcsii, ncm as rncm
    from signal_processing.gammatone import GammatoneFilterbank
    out = {}
    f64 = lambda s: s.astype(np.float64)

    # ---- CSII ----
    for fs in (8000, 16000, 22050):
        out["sii.%d" % fs] = rcsii._speech_importance_function(129, fs, 256)
    for name, fs, L, seed in ic.CSII_CASES:
        c, e = (f64(s) for s in ic.pair(L, seed, fs))
        frame = int(0.016 * fs)
        out["csii." + name] = np.float64(rcsii.compute_csii(c, e, fs))
        out["csii.ident." + name] = np.float64(rcsii.compute_csii(c, c, fs))
        out["msc." + name] = rcsii._magnitude_squared_coherence(c, e, fs, frame, frame // 2, 256)
        got = ic.msc64(c, e, fs, want_den=True)
        if got is not None:
            assert bool(((got[1] == 0) | (got[1] > 1e-6)).all()), (name, float(got[1].min()))
        print("%s fs %d L %d -> csii %.6f (identical pair %.6f)" % (name, fs, L, out["csii." + name], out["csii.ident." + name]))
    for fs, lengths in ic.CSII_GOLDEN_LENGTHS.items():                       # property 1
        frame = int(0.016 * fs)
        vals = []
        for i, L in enumerate(lengths):
            c, e = (f64(s) for s in ic.pair(L, 540 + i, fs))
            msc = rcsii._magnitude_squared_coherence(c, e, fs, frame, frame // 2, 256)
            want = 0.0 if L < frame else float(np.clip(np.sum(out["sii.%d" % fs] * msc), 0, 1))
            for levels in (1, 3, 5):
                got = float(rcsii.compute_csii(c, e, fs, num_levels=levels))
                assert abs(got - want) <= 1e-15, (fs, L, levels, got, want)
            vals.append(want)
        out["csii.len.%d" % fs] = np.asarray(vals)
        print("property 1 holds at fs %d, lengths %s" % (fs, lengths))

    # ---- Hilbert ----
    for L in (64, 65, 401, 1237, 2000):                                       # property 2
        x = f64(ic.hilbert_rows(L))
        err = np.abs(ic.hilbert64(x)[0] - hilbert(x).imag).max()
        assert err <= 5e-15, (L, err)
        if L in (64, 65):
            out["hilbert.h%d" % L] = hilbert(np.eye(1, L)[0]).imag
            out["hilbert.y%d" % L] = hilbert(x).imag
    print("property 2 holds")

    # ---- NCM ----
    banks = {name: GammatoneFilterbank(**kw) for name, kw in ic.BANKS.items()}
    for name, bname, fs, L, seed in ic.NCM_CASES:
        c, e = (f64(s) for s in ic.pair(L, seed, fs))
        b = banks[bname]
        out["ncm." + name] = np.float64(rncm.compute_ncm(c, e, fs, gfb=b))
        ncc = np.zeros(b.num_channels)
        if L >= 64:
            cf, ef = b.filter(c), b.filter(e)
            ncc = np.asarray([rncm._normalized_covariance(rncm._compute_envelope(cf[i]), rncm._compute_envelope(ef[i]))
                              for i in range(b.num_channels)], dtype=np.float64)
            den = ic.ncm_denominators(c, e, ic.bank(bname))
            assert bool(((den == 0) | (den > 1e-6)).all()), (name, float(den.min()))
        out["ncc." + name] = ncc
        print("%s L %d -> ncm %.6f" % (name, L, out["ncm." + name]))
    keep = rncm._normalized_covariance
    try:
        for bname, b in banks.items():
            c, e = (f64(s) for s in ic.pair(64, 1, 8000))
            w = np.zeros(b.num_channels)
            for i in range(b.num_channels):
                calls = []
                rncm._normalized_covariance = lambda x, y: (calls.append(0), 1.0 if len(calls) - 1 == i else 0.0)[1]
                w[i] = rncm.compute_ncm(c, e, 8000, gfb=b)
            out["chw." + bname] = w
    finally:
        rncm._normalized_covariance = keep

    path = os.path.join(HERE, "g21_intelligibility.npz")
    np.savez_compressed(path, **out)
    print("g21_intelligibility %.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
