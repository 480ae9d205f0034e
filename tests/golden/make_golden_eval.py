"""Generator of tests/golden/g14_eval.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), like
make_golden.py: imports the reference's evaluation functions - never shipped, never copied - and stores what they return on
the pairs of tests/eval_cases.py: compute_ssnr, compute_stoi (its fallback: pystoi is not installed) and _pesq_simplified (what
compute_pesq returns without the pesq package) of every pair, 36 doubles, plus the identical pair.

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_eval: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import eval_cases as ec  # noqa: E402


def main():
    from evaluation.ssnr import compute_ssnr
    from evaluation.stoi import compute_stoi
    from evaluation.pesq_eval import _pesq_simplified
    clean, _, enh = ec.signals()
    ic, ie = ec.identical_pair()

    def three(c, e):
        n = min(len(c), len(e))
        return (np.float64(compute_ssnr(c, e, ec.FS)), np.float64(compute_stoi(c, e, ec.FS)),
                np.float64(_pesq_simplified(c[:n].astype(np.float64), e[:n].astype(np.float64), ec.FS)))
    rows = np.array([three(c, e) for c, e in zip(clean, enh)])
    ident = np.array(three(ic, ie))
    out = {"lengths": np.asarray(ec.LENGTHS, dtype=np.int64), "ssnr": rows[:, 0], "stoi": rows[:, 1], "pesq": rows[:, 2],
           "identical": ident}
    path = os.path.join(HERE, "g14_eval.npz")
    np.savez_compressed(path, **out)
    for k in ("ssnr", "stoi", "pesq", "identical"):
        print(k, np.array2string(out[k], precision=4, max_line_width=200))
    print("g14_eval %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
