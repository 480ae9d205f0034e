"""Generator of tests/golden/g19_gammatone.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), on
the CPU: imports the reference's signal_processing/gammatone.py - never shipped, never copied - and stores what it returns on the
seeded cases of tests/gammatone_cases.py.

  <bank>.center_freqs          erb_space of each filterbank configuration of gammatone_cases.BANKS (float64)
  <bank>.taps                  the tap count
  default.ir<c>                gammatone_impulse_response of channels 0, 31 and 63 of the default bank (float64)
  erb_bandwidth                erb_bandwidth(center_freqs) of the default bank
  <case>.mag / .phase          GammatoneFilterbank.get_tf_magnitudes of the case signal with the case's framing (float64 [C, T])
  filter.<case>                rows GOLDEN_FILTER[1] of GammatoneFilterbank.filter of one short case signal (float64)

It also asserts, for EVERY case (stored or not), that the phase row of tests/test_gammatone_gpu.py skips at most 1 % of the units.

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gammatone.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_gammatone: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import gammatone_cases as gc  # noqa: E402


def main():
    from signal_processing.gammatone import GammatoneFilterbank, erb_bandwidth, gammatone_impulse_response
    out = {}
    banks = {name: GammatoneFilterbank(**kw) for name, kw in gc.BANKS.items()}
    for name, b in banks.items():
        out[name + ".center_freqs"] = b.center_freqs
        out[name + ".taps"] = np.int64(len(b.impulse_responses[0]))
    for c in (0, 31, 63):
        out["default.ir%d" % c] = gammatone_impulse_response(banks["default"].center_freqs[c], 8000)
        assert np.array_equal(out["default.ir%d" % c], banks["default"].impulse_responses[c])
    out["erb_bandwidth"] = erb_bandwidth(banks["default"].center_freqs)
    for name in gc.GOLDEN_CASES:
        _, bname, L, _, _, (frame, hop, N) = gc.CASES[name]
        mag, phase = banks[bname].get_tf_magnitudes(gc.case_signal(name).numpy().astype(np.float64), frame, hop, N)
        out[name + ".mag"], out[name + ".phase"] = mag, phase
        print("%s L %d -> %s, mean power %.3e" % (name, L, mag.shape, mag.mean()))
    fname, rows = gc.GOLDEN_FILTER
    y = banks[gc.CASES[fname][1]].filter(gc.case_signal(fname).numpy().astype(np.float64))
    out["filter." + fname] = y[list(rows)]
    import torch
    for name in gc.CASES:
        bound, keep, skipped = gc.phase_bound(name)
        a64 = gc.analysis(name, torch.float64)
        live = gc.live_units(a64["norm"])
        small = float((torch.sqrt(a64["re"] ** 2 + a64["im"] ** 2) / a64["norm"].clamp_min(1e-300))[live].min())
        print("%s: smallest |S[cf_bin]| / sqrt(w sum f^2) %.4f, largest phase bound %.2e rad, %d of %d units skipped, %d silent "
              "or dead, silent frames %s" % (name, small, float(bound.max()), skipped, keep.numel(), int((~live).sum()),
                                             gc.silent_frames(name)))
        assert skipped <= 0.01 * keep.numel(), name
    path = os.path.join(HERE, "g19_gammatone.npz")
    np.savez_compressed(path, **out)
    print("g19_gammatone %.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
