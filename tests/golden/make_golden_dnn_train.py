"""Generator of tests/golden/g25_dnn_train.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), on the
CPU: imports the reference's training/pipeline.py, signal_processing/features.py and models/dnn.py - never shipped, never copied - and
stores what they return, data only, on the seeded frame set of tests/dnn_train_cases.py.

  lengths                      frames per utterance (1, 3, 11, 12, 130)
  ds.feat_mean / ds.feat_std   SpeechEnhancementDataset's statistics over the add_context rows of the five utterances, float32 [594]
  ds.features / ds.masks       its normalised, clipped rows [157, 594] and clipped masks [157, 64]
  ds2.*                        the same of a second Dataset (utterances 0 .. 2) built with the first one's statistics
  loss, norm                   per step of two epochs of the reference's _train_epoch on the CPU (use_amp false), dropout p = 0, an
                               unshuffled loader of batch 37 (37, 37, 37, 37, 9), Adam(lr 1e-3, weight_decay 1e-5), clip 5.0: the loss
                               and clip_grad_norm_'s total norm before clipping
  step<k>.<key>                every parameter after step k = 1, 2, 5, 10 and the last; network.0.weight at the columns
                               dnn_cases.GRAD_COLS only (the fixture stays under 1 MiB)
  train_loss, val_loss         what _train_epoch and _validate (on the second Dataset) returned per epoch

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dnn_train.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_dnn_train: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

SNAPSHOTS = (1, 2, 5, 10)


def main():
    import torch
    from torch.utils.data import DataLoader
    import dnn_cases as dn
    import dnn_train_cases as tc
    from models.dnn import SpeechEnhancementDNN
    from signal_processing.features import FeatureExtractor
    from training.pipeline import SpeechEnhancementDataset, TrainingPipeline

    out = {"lengths": np.asarray(tc.LENGTHS, dtype=np.int64)}
    raws, masks = tc.frame_set()
    fe = FeatureExtractor()
    assert fe.context == dn.CTX
    rows = [fe.add_context(r) for r in raws]
    ds = SpeechEnhancementDataset(rows, masks)
    ds2 = SpeechEnhancementDataset(rows[:3], masks[:3], feat_mean=ds.feat_mean, feat_std=ds.feat_std)
    for name, d in (("ds", ds), ("ds2", ds2)):
        out[name + ".feat_mean"], out[name + ".feat_std"] = np.asarray(d.feat_mean), np.asarray(d.feat_std)
        out[name + ".features"], out[name + ".masks"] = d.features.numpy().copy(), d.masks.numpy().copy()
    assert len(ds) == tc.N_FRAMES and (out["ds.feat_std"][:15] == 1.0).all()

    Ws, bs = tc.fixture_params()
    model = SpeechEnhancementDNN(input_dim=dn.SMALL[0], hidden_dim=dn.SMALL[1], output_dim=dn.SMALL[-1], num_hidden_layers=len(dn.SMALL) - 2)
    model.load_state_dict(dn.state_dict(Ws, bs))
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    pipe = object.__new__(TrainingPipeline)                # its constructor creates directories; the two methods need these three
    pipe.model, pipe.device, pipe.use_amp = model, torch.device("cpu"), False
    optimizer = torch.optim.Adam(model.parameters(), lr=tc.LR, weight_decay=tc.WD)
    criterion = torch.nn.MSELoss()
    losses, norms, snaps = [], [], {}

    def recording_criterion(pred, target):
        loss = criterion(pred, target)
        if torch.is_grad_enabled():
            losses.append(float(loss))
        return loss

    clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(params, max_norm):
        assert max_norm == tc.MAX_NORM
        total = clip(params, max_norm)
        norms.append(float(total))
        return total

    step = optimizer.step

    def recording_step(*a, **k):
        r = step(*a, **k)
        if len(norms) in SNAPSHOTS:
            snaps[len(norms)] = {k_: v.detach().numpy().copy() for k_, v in model.state_dict().items()}
        return r

    torch.nn.utils.clip_grad_norm_ = recording_clip
    optimizer.step = recording_step
    train_loader = DataLoader(ds, batch_size=tc.BATCH, shuffle=False)
    test_loader = DataLoader(ds2, batch_size=tc.BATCH, shuffle=False)
    train_losses, val_losses = [], []
    for _ in range(2):
        train_losses.append(pipe._train_epoch(train_loader, optimizer, recording_criterion, None))
        val_losses.append(pipe._validate(test_loader, recording_criterion))
    torch.nn.utils.clip_grad_norm_ = clip
    snaps[len(norms)] = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    assert len(losses) == len(norms) == 10, (len(losses), len(norms))
    norms_a = np.asarray(norms)
    print("gradient norms:", np.round(norms_a, 4))
    assert (np.abs(norms_a / tc.MAX_NORM - 1.0) > 0.01).all(), "a norm within 1 % of the clip"
    assert (norms_a > tc.MAX_NORM).any(), "no step is clipped"
    out["loss"], out["norm"] = np.asarray(losses), norms_a
    out["train_loss"], out["val_loss"] = np.asarray(train_losses), np.asarray(val_losses)
    out["snapshots"] = np.asarray(sorted(snaps), dtype=np.int64)
    for k, sd in snaps.items():
        for key, v in sd.items():
            out["step%d.%s" % (k, key)] = v[:, dn.GRAD_COLS] if key == "network.0.weight" else v
    path = os.path.join(HERE, "g25_dnn_train.npz")
    np.savez_compressed(path, **out)
    print("g25_dnn_train %.1f KB, %d arrays, losses %s" % (os.path.getsize(path) / 1024, len(out), np.round(losses, 5)))
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
