"""Generator of tests/golden/g22_dnn.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), on the CPU:
imports the reference's models/dnn.py - never shipped, never copied - and stores what it returns, data only, on the seeded cases
of tests/dnn_cases.py.

  state.<key>            the small model's state (input 594, hidden 64 x 3, output 64; dnn_cases.params(SMALL, GOLDEN_SEED) loaded
                         into the reference's module and read back), float32
  y                      its eval() outputs on the 37 rows dnn_cases.inputs(37, 594, GOLDEN_SEED + 1), float32
  grad.<key>             eval-mode autograd gradients of nn.MSELoss against dnn_cases.targets(37, 64, GOLDEN_SEED + 2), float32;
                         network.0.weight's at the columns dnn_cases.GRAD_COLS only (the fixture stays under 400 KB)
  grad_cols              those columns
  rbm.<key>              the state after load_rbm_weights on the seeded tuples dnn_cases.rbm_tuples(): biases whole, weights at [::4, ::4];
                         four tuples are handed over, so that the output layer's must be ignored
  default.keys / default.shapes / default.count     the DEFAULT model's state_dict keys, shapes and count_parameters()
  or_defaults            (input_dim, hidden_dim, output_dim, num_hidden_layers, dropout_rate) of SpeechEnhancementDNN(0, 0, 0, 0, 0)

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dnn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_dnn: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

def main():
    import torch
    import dnn_cases as dn
    from models.dnn import SpeechEnhancementDNN
    out = {}
    Ws, bs = dn.params(dn.SMALL, dn.GOLDEN_SEED)
    m = SpeechEnhancementDNN(input_dim=dn.SMALL[0], hidden_dim=dn.SMALL[1], output_dim=dn.SMALL[-1], num_hidden_layers=len(dn.SMALL) - 2)
    m.load_state_dict(dn.state_dict(Ws, bs))
    m.eval()
    for k, v in m.state_dict().items():
        out["state." + k] = v.numpy().copy()
    x = torch.from_numpy(dn.inputs(dn.SMALL_ROWS, dn.SMALL[0], dn.GOLDEN_SEED + 1))
    t = torch.from_numpy(dn.targets(dn.SMALL_ROWS, dn.SMALL[-1], dn.GOLDEN_SEED + 2))
    y = m(x)
    out["y"] = y.detach().numpy().copy()
    torch.nn.MSELoss()(y, t).backward()
    for k, p in m.named_parameters():
        g = p.grad.numpy().copy()
        out["grad." + k] = g[:, dn.GRAD_COLS] if k == "network.0.weight" else g
    out["grad_cols"] = dn.GRAD_COLS.astype(np.int64)
    before = m.state_dict()["network.9.weight"].numpy().copy()
    m.load_rbm_weights(dn.rbm_tuples(dn.SMALL, dn.GOLDEN_SEED + 3))
    for k, v in m.state_dict().items():
        out["rbm." + k] = v.numpy().copy() if v.dim() == 1 else v.numpy()[::4, ::4].copy()
    assert np.array_equal(m.state_dict()["network.9.weight"].numpy(), before)
    d = SpeechEnhancementDNN()
    sd = d.state_dict()
    out["default.keys"] = np.array(list(sd))
    out["default.shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], dtype=np.int64)
    out["default.count"] = np.int64(d.count_parameters())
    z = SpeechEnhancementDNN(0, 0, 0, 0, 0)
    out["or_defaults"] = np.array([z.input_dim, z.hidden_dim, z.output_dim, z.num_hidden_layers, z.dropout_rate], dtype=np.float64)
    path = os.path.join(HERE, "g22_dnn.npz")
    np.savez_compressed(path, **out)
    print("g22_dnn %.1f KB, %d arrays, default count %d" % (os.path.getsize(path) / 1024, len(out), int(out["default.count"])))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
