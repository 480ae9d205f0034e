"""Mirror of masks/pcirm.py: the Phase Correlation Ideal Ratio Mask on device tensors (csrc/masks.hip)."""
from .. import ops
from ._device import planes


def compute_correlation_coefficients(noisy_frames, clean_frames, noise_frames, eps=1e-10):
    """masks/pcirm.py:22-74 -> (rho_s, rho_n).  The device version ALWAYS applies the per-T-F-unit rule of the reference's
    `ndim == 2` branch, |a b| / (sqrt(a^2 + eps) sqrt(b^2 + eps)) clipped to [0, 1], at every element, whatever the rank.
    The reference sums over the last axis when `ndim == 3`; here a [B, T, F] batch gives what the reference gives when it is
    called on each x[b]."""
    y, c, n = planes("compute_correlation_coefficients", noisy_frames, clean_frames, noise_frames)
    return ops.mask_corr(y, c, n, eps)


def compute_phase_differences(noisy_phase, clean_phase, noise_phase):
    """masks/pcirm.py:77-95 -> (phi1, phi2) = (clean - noisy, noise - noisy)"""
    y, c, n = planes("compute_phase_differences", noisy_phase, clean_phase, noise_phase)
    return c - y, n - y


def compute_pcirm(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2, eps=1e-10):
    """masks/pcirm.py:98-133: rho_s (c |cos phi1|)^2 / (rho_s (c |cos phi1|)^2 + rho_n (n |cos phi2|)^2 + eps), clipped"""
    return ops.mask_pcirm(*planes("compute_pcirm", clean_mag, noise_mag, rho_s, rho_n, phi1, phi2), eps)


def compute_pcirm_from_signals(noisy_frames, clean_frames, noise_frames, noisy_phase, clean_phase, noise_phase, clean_mag,
                               noise_mag, eps=1e-10):
    """masks/pcirm.py:136-164 -> (pcirm, rho_s, rho_n, phi1, phi2)"""
    rho_s, rho_n = compute_correlation_coefficients(noisy_frames, clean_frames, noise_frames, eps)
    phi1, phi2 = compute_phase_differences(noisy_phase, clean_phase, noise_phase)
    return compute_pcirm(clean_mag, noise_mag, rho_s, rho_n, phi1, phi2, eps), rho_s, rho_n, phi1, phi2
