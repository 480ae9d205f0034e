"""Generator of tests/golden/g16_adversarial.npz and g16_adversarial_state.json.  Runs ONLY where the reference is checked out
(SFM_REFERENCE names its root), like make_golden_losses.py, on the CPU: imports the reference's AdversarialLoss - never shipped,
never copied - and stores seeds and results only, on the cases of tests/adversarial_cases.py:
  state json: per input_dim of the cases, per state_dict key, the shape, the float64 sum and the first 8 values after the seeded
              default init (the whole state is 8 MB), and the parameter count;
  npz:        per case and objective (d, g, fm; each from a fresh seeded module in train()): the fp32 loss, the gradient to
              `enhanced` (g, fm), the float64 sum of every parameter's gradient in named_parameters() order (NaN where it gets none: the heads under fm), and weight_u /
              weight_v of every discriminator's first conv after the calls.

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adversarial.py
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
    raise SystemExit("make_golden_adversarial: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import adversarial_cases as ac  # noqa: E402


def main():
    from training.losses import AdversarialLoss

    def fresh(input_dim):
        torch.manual_seed(ac.INIT_SEED)
        return AdversarialLoss(input_dim=input_dim).train()

    states = {}
    for dim in sorted({c[0] for c in ac.CASES.values()}):
        m = fresh(dim)
        states[str(dim)] = {"parameters": len(list(m.parameters())), "elements": sum(p.numel() for p in m.parameters()),
                            "keys": {k: ac.summary(v) for k, v in m.state_dict().items()}}
    with open(os.path.join(HERE, "g16_adversarial_state.json"), "w") as f:
        json.dump(states, f, indent=0)
        f.write("\n")
    out = {}
    for name, (dim, B, T, seed) in ac.CASES.items():
        c = ac.case(name)
        out[name + ".seed"] = np.int64(seed)
        for mode in ac.MODES:
            m = fresh(dim)
            e = c["enh"].clone().requires_grad_(True)
            loss = {"d": lambda: m.discriminator_loss(c["clean"], e), "g": lambda: m.generator_loss(e),
                    "fm": lambda: m.feature_matching_loss(c["clean"], e)}[mode]()
            loss.backward()
            pre = "%s.%s." % (name, mode)
            out[pre + "loss"] = loss.detach().numpy()
            if mode != "d":
                out[pre + "grad"] = e.grad.numpy()
            assert mode != "d" or e.grad is None
            names = [k for k, _ in m.named_parameters()]
            out[pre + "pgrad_sums"] = np.array([float("nan") if p.grad is None else float(p.grad.double().sum()) for _, p in m.named_parameters()])
            out[pre + "pgrad_norms"] = np.array([float("nan") if p.grad is None else float(p.grad.double().norm()) for _, p in m.named_parameters()])
            sd = m.state_dict()
            for i in range(3):
                for k in ("weight_u", "weight_v"):
                    out["%su%d.%s" % (pre, i, k)] = sd["discriminators.%d.layers.0.%s" % (i, k)].numpy()
            print("%-18s %-2s loss %.7f" % (name, mode, float(loss.detach())))
        out[name + ".param_names"] = np.array(names)
    path = os.path.join(HERE, "g16_adversarial.npz")
    np.savez_compressed(path, **out)
    print("g16_adversarial %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
