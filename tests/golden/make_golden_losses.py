"""Generator of tests/golden/g15_losses.npz and g15_curriculum.json.  Runs ONLY where the reference is checked out
(SFM_REFERENCE names its root), like make_golden.py, on the CPU: imports the reference's PerceptualSTOILoss, MSEMaskLoss and
CurriculumScheduler - never shipped, never copied - and stores what they return on the seeded cases of tests/loss_cases.py:
the fp32 loss and its autograd gradient to the enhanced magnitudes (of c7 the last utterance's rows only: the whole is 4 MB),
the two band matrices, one MSE value with its gradient, and get_stage(e) of epochs 0..49.  Seeds and outputs only; the
inputs are rebuilt from the seeds.

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_losses.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_losses: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import loss_cases as lc  # noqa: E402

MSE_SHAPE, MSE_SEED = (2, 61, 129), 161


def main():
    from training.losses import MSEMaskLoss, PerceptualSTOILoss
    from training.curriculum import CurriculumScheduler
    torch.manual_seed(0)
    mods = {8000: PerceptualSTOILoss(8000), 16000: PerceptualSTOILoss(16000)}
    out = {"band_weights_8000": mods[8000].band_weights.numpy(), "band_weights_16000": mods[16000].band_weights.numpy()}
    for name in lc.FIXTURE_CASES:
        c = lc.case(name)
        e = c["enh"].clone().requires_grad_(True)
        loss = mods[lc.CASES[name][3]](e, c["clean"])
        loss.backward()
        out[name + ".seed"] = np.int64(lc.CASES[name][4])
        out[name + ".loss"] = loss.detach().numpy()
        out[name + ".grad"] = e.grad[lc.FIXTURE_GRAD_ROWS.get(name, slice(None))].numpy()
        print("%-20s loss %.7f  grad %s" % (name, float(loss), tuple(out[name + ".grad"].shape)))
    p, t = lc.mse_case(MSE_SHAPE, MSE_SEED)
    p.requires_grad_(True)
    loss = MSEMaskLoss()(p, t)
    loss.backward()
    out["mse.seed"], out["mse.loss"], out["mse.grad"] = np.int64(MSE_SEED), loss.detach().numpy(), p.grad.numpy()
    path = os.path.join(HERE, "g15_losses.npz")
    np.savez_compressed(path, **out)
    print("g15_losses %.1f KB" % (os.path.getsize(path) / 1024))
    sched = CurriculumScheduler()
    with open(os.path.join(HERE, "g15_curriculum.json"), "w") as f:
        json.dump({"total_epochs": sched.total_epochs, "stages": [sched.get_stage(e) for e in range(50)]}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
