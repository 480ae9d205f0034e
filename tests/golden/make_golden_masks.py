"""Generator of tests/golden/g17_masks.npz.  Runs ONLY where the reference is checked out (SFM_REFERENCE names its root), like
make_golden_losses.py, on the CPU: imports the reference's masks/ and _add_noise_at_snr - never shipped, never copied - and
stores what they return on the seeded cases of tests/mask_cases.py.

  u<k>.clean / .noise      the waveforms of utterance k (float32)
  u<k>.noisy               _add_noise_at_snr(clean, noise, snr)
  u<k>.scale               the scale it used, recovered from its result: <noisy - clean, tiled noise> / <tiled, tiled> in float64
  u<k>.irm / .pcirm / .opt / .opt_mid
                           compute_irm, compute_pcirm (with compute_correlation_coefficients and compute_phase_differences)
                           and quantize_pcirm without / with middle_value on np.abs / np.angle of the reference's batch_stft
                           of the clean utterance, of the scaled noise and of the mix, per utterance [T, F]
  r<j>.irm / .irm_p / .rho_s / .rho_n / .pcirm / .opt / .opt_mid
                           the same functions on the float32 random planes of mask_cases.random_case (rebuilt from the seed)
  steps, exponent          compute_snr_boundaries()

    SFM_REFERENCE=<reference root> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_masks.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SFM_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("make_golden_masks: set SFM_REFERENCE to the reference's root")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import mask_cases as mc  # noqa: E402


def main():
    from masks.irm import compute_irm
    from masks.pcirm import compute_correlation_coefficients, compute_pcirm, compute_phase_differences
    from masks.opt_pcirm import compute_snr_boundaries, quantize_pcirm
    from training.conformer_pipeline import _add_noise_at_snr, batch_stft
    steps, exponent = compute_snr_boundaries()
    out = {"steps": steps, "exponent": np.float64(exponent), "middle_value": np.float64(mc.MIDDLE_VALUE)}

    def spec(x):
        re, im = batch_stft(torch.from_numpy(x).unsqueeze(0), mc.FFT, mc.HOP, mc.WIN)
        return (re[0] + 1j * im[0]).numpy()

    for k, (L, Ln, snr, seed) in enumerate(mc.UTTERANCES):
        clean, noise = (t.numpy() for t in mc.utterance(k))
        noisy = _add_noise_at_snr(clean, noise, snr)
        tiled = np.tile(noise, int(np.ceil(L / Ln)))[:L].astype(np.float64)
        scale = float(((noisy.astype(np.float64) - clean) * tiled).sum() / (tiled * tiled).sum())
        C, sN, Y = spec(clean), spec((scale * tiled).astype(np.float32)), spec(noisy)
        cm, nm, ym = np.abs(C), np.abs(sN), np.abs(Y)
        rho_s, rho_n = compute_correlation_coefficients(ym, cm, nm)
        phi1, phi2 = compute_phase_differences(np.angle(Y), np.angle(C), np.angle(sN))
        pc = compute_pcirm(cm, nm, rho_s, rho_n, phi1, phi2)
        u = "u%d." % k
        out.update({u + "clean": clean, u + "noise": noise, u + "noisy": noisy, u + "scale": np.float64(scale),
                    u + "seed": np.int64(seed), u + "irm": compute_irm(cm, nm), u + "pcirm": pc,
                    u + "opt": quantize_pcirm(pc, steps), u + "opt_mid": quantize_pcirm(pc, steps, middle_value=mc.MIDDLE_VALUE)})
        assert all(out[u + n].dtype == np.float32 for n in ("noisy", "irm", "pcirm", "opt", "opt_mid"))
        print("%s L %d frames %d scale %.6f  irm mean %.3f pcirm mean %.3f" % (u, L, cm.shape[0], scale, out[u + "irm"].mean(),
                                                                            pc.mean()))
    for name in mc.RANDOM:
        c = {k: v.numpy() for k, v in mc.random_case(name).items()}
        rho_s, rho_n = np.stack([compute_correlation_coefficients(c["ym"][b], c["cm"][b], c["nm"][b])
                                 for b in range(c["ym"].shape[0])], axis=1)
        phi1, phi2 = compute_phase_differences(c["py"], c["pc"], c["pn"])
        r = name + "."
        with np.errstate(invalid="ignore"):
            out.update({r + "seed": np.int64(mc.RANDOM[name][1]), r + "irm": compute_irm(c["cm"], c["nm"]),
                        r + "irm_p": compute_irm(c["cm"], c["nm"], p=0.3), r + "rho_s": rho_s, r + "rho_n": rho_n,
                        r + "pcirm": compute_pcirm(c["cm"], c["nm"], c["rho_s"], c["rho_n"], phi1, phi2),
                        r + "opt": quantize_pcirm(c["q"], steps),
                        r + "opt_mid": quantize_pcirm(c["q"], steps, middle_value=mc.MIDDLE_VALUE)})
        assert all(out[r + n].dtype == np.float32 and out[r + n].shape == c["cm"].shape
                   for n in ("irm", "irm_p", "rho_s", "rho_n", "pcirm", "opt", "opt_mid"))
    path = os.path.join(HERE, "g17_masks.npz")
    np.savez_compressed(path, **out)
    print("g17_masks %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
