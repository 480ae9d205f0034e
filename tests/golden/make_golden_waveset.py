"""Generator of tests/golden/g26_waveset.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), on the
CPU: imports the reference's training/conformer_pipeline.py - never shipped, never copied - replaces its _load_audio by a lookup
into the seeded signals of tests/waveset_cases.py at run time, and stores what its own WaveformDataset and train() give, data only.

  lengths, entry<i>, noise<k>  the inputs: samples per entry of the file list (-1: a file whose load raises), the signals
  snr_levels, fs, max_len      config.SNR_LEVELS of the reference, 8000, 2000
  kept                         the positions in the file list of the utterances WaveformDataset kept
  noisy, clean                 every ds[i] pair, [N, max_len] each
  mult<total>                  lr_lambda(0 .. total - 1) of the closure train(epochs=total) hands to LambdaLR, total in
                               waveset_cases.TOTALS: LambdaLR is replaced by a recorder that stops the run
  epochs0_total                the total_epochs of that closure for train(epochs=0)

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_waveset.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_waveset: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)


class _Stop(Exception):
    pass


def main():
    import torch
    import waveset_cases as wc
    import config as ref_config
    from training import conformer_pipeline as ref

    entries, noises = wc.make_inputs()
    table = {"entry%d" % i: e for i, e in enumerate(entries)}

    def lookup(path, target_sr=None):
        if table[path] is None:
            raise IOError("no such file: %s" % path)
        return table[path]

    ref._load_audio = lookup
    noise_signals = {"noise%d" % k: z for k, z in enumerate(noises)}
    snr_levels = list(ref_config.SNR_LEVELS)
    ds = ref.WaveformDataset(list(table), noise_signals, snr_levels, wc.FS, max_len=wc.MAX_LEN)
    pairs = [ds[i] for i in range(len(ds))]
    noisy = np.stack([p[0].numpy() for p in pairs])
    clean = np.stack([p[1].numpy() for p in pairs])
    assert noisy.dtype == np.float32 and noisy.shape == (len(wc.KEPT), wc.MAX_LEN)
    # the kept positions, from the data itself: each kept clean row is the head of exactly one entry
    kept = [i for i, e in enumerate(entries) if e is not None and len(e) >= ref_config.FRAME_SIZE * 4]
    assert tuple(kept) == wc.KEPT and ref_config.FRAME_SIZE * 4 == wc.MIN_LEN
    for row, i in zip(clean, kept):
        n = min(len(entries[i]), wc.MAX_LEN)
        assert np.array_equal(row[:n], entries[i][:n]) and not row[n:].any()

    # only a non-stationary utterance tells the full-length scale from the scale of the cut utterance
    nid, snr = wc.LONG % len(noises), snr_levels[wc.LONG % len(snr_levels)]
    s_full = wc.mix_scale(entries[wc.LONG], noises[nid], snr)
    s_cut = wc.mix_scale(entries[wc.LONG], noises[nid], snr, mutant=wc.MUTANTS[1])
    print("entry %d: scale over the full length %.6f, after the cut %.6f" % (wc.LONG, s_full, s_cut))
    assert abs(s_cut / s_full - 1.0) > 0.30

    out = {"lengths": np.asarray([-1 if n is None else n for n in wc.ENTRY_LENGTHS], dtype=np.int64),
           "snr_levels": np.asarray(snr_levels, dtype=np.float64), "fs": np.int64(wc.FS), "max_len": np.int64(wc.MAX_LEN),
           "kept": np.asarray(kept, dtype=np.int64), "noisy": noisy, "clean": clean}
    for i, e in enumerate(entries):
        if e is not None:
            out["entry%d" % i] = e
    for k, z in enumerate(noises):
        out["noise%d" % k] = z

    # the schedule: the closure that train() itself builds
    pipe = object.__new__(ref.ConformerPipeline)            # (its constructor creates directories)
    pipe.fs, pipe.fft_size, pipe.hop_size, pipe.frame_size = wc.FS, ref_config.FFT_SIZE, ref_config.HOP_SIZE, ref_config.FRAME_SIZE
    pipe.device, pipe.use_amp, pipe.model = torch.device("cpu"), False, None
    seen = []

    def recorder(optimizer, lr_lambda, *a, **k):
        seen.append(lr_lambda)
        raise _Stop()

    real = torch.optim.lr_scheduler.LambdaLR
    torch.optim.lr_scheduler.LambdaLR = recorder
    try:
        for total in wc.TOTALS + (0,):
            try:
                pipe.train(None, None, epochs=total)
            except _Stop:
                pass
            fn = seen[-1]
            cells = dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))
            if total:
                assert cells["total_epochs"] == total
                out["mult%d" % total] = np.asarray([fn(e) for e in range(total)], dtype=np.float64)
            else:
                out["epochs0_total"] = np.int64(cells["total_epochs"])
    finally:
        torch.optim.lr_scheduler.LambdaLR = real
    assert len(seen) == len(wc.TOTALS) + 1 and int(out["epochs0_total"]) == 50

    path = os.path.join(HERE, "g26_waveset.npz")
    np.savez_compressed(path, **out)
    print("g26_waveset %.1f KB, %d arrays" % (os.path.getsize(path) / 1024, len(out)))
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
