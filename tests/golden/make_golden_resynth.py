"""Generator of tests/golden/g23_resynth.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), on the
CPU: constructs the reference's training/pipeline.py TrainingPipeline - never shipped, never copied - sets its `model` to a stub
nn.Module that returns prescribed rows of the seeded mask of tests/resynth_cases.py whatever features it is handed, leaves
feat_mean / feat_std unset and stores what enhance_signal returns, data only.  The reference's own FeatureExtractor runs (its rows
only decide how many rows the stub is asked for); steps 2-4 are the reference's code.  The directories the constructor creates are
pointed at a temporary directory first.

  out.<L>               enhance_signal's float32 output for the noisy signal resynth_cases.case("default", L, GOLDEN_SEED + i) at 8 kHz,
                        L = 159, 160, 239, 240, 241, 1237, the stub returning one mask row per STFT frame (one row where there is none)
  out.short             L = 1237 with the stub returning two rows fewer than the STFT has frames
  cf, bin_freqs         the np.interp table's inputs: erb_space(FREQ_LOW, FREQ_HIGH, NUM_CHANNELS) and np.linspace(0, fs / 2, 129), float64
  interp.mask, interp.g one seeded mask row and np.interp(bin_freqs, cf, row, left=row[0], right=row[-1]), float64
  hann                  np.hanning(160), float64

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resynth.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_resynth: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

GOLDEN_SEED = 900


def main():
    import torch
    import resynth_cases as rc
    import config as ref_config
    from signal_processing.gammatone import erb_space

    class Stub(torch.nn.Module):
        """returns the prescribed rows, whatever the batch"""

        def __init__(self, rows):
            super().__init__()
            self.rows = torch.from_numpy(np.ascontiguousarray(rows))

        def forward(self, batch):
            return self.rows

    with tempfile.TemporaryDirectory() as tmp:
        ref_config.BASE_DIR = tmp
        ref_config.MODEL_DIR = os.path.join(tmp, "models")
        from training.pipeline import TrainingPipeline
        tp = TrainingPipeline(mask_type="pcirm", use_rbm_pretrain=False)
        tp.device = torch.device("cpu")
        tp.use_amp = False
        assert tp.feat_mean is None and tp.feat_std is None and tp.fs == 8000
        out = {}
        todo = [("out.%d" % L, L, GOLDEN_SEED + i, 0) for i, L in enumerate(rc.GOLDEN_LENGTHS)]
        todo.append(("out.short", rc.GOLDEN_SHORT[0], GOLDEN_SEED + 20, rc.GOLDEN_SHORT[1]))
        for key, L, seed, dT in todo:
            noisy, mask = rc.case("default", L, seed, dT)
            tp.model = Stub(mask)
            y = tp.enhance_signal(noisy.copy())
            assert y.dtype == np.float32 and y.shape == (L,)
            out[key] = y
    cf = np.asarray(erb_space(ref_config.FREQ_LOW, ref_config.FREQ_HIGH, ref_config.NUM_CHANNELS), dtype=np.float64)
    freqs = np.linspace(0, tp.fs / 2, ref_config.FFT_SIZE // 2 + 1)
    row = rc.case("default", 1237, GOLDEN_SEED + 5)[1][3].astype(np.float64)
    out.update({"cf": cf, "bin_freqs": freqs, "interp.mask": row, "interp.g": np.interp(freqs, cf, row, left=row[0], right=row[-1]),
                "hann": np.hanning(ref_config.FRAME_SIZE).astype(np.float64)})
    path = os.path.join(HERE, "g23_resynth.npz")
    np.savez_compressed(path, **out)
    print("g23_resynth %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
