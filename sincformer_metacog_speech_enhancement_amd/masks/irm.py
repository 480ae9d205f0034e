"""Mirror of masks/irm.py: the Ideal Ratio Mask on device tensors (csrc/masks.hip, sfm_mask_irm)."""
from .. import ops
from ._device import planes


def compute_irm(clean_mag, noise_mag, p=0.5, eps=1e-10):
    """masks/irm.py:17-39.  clip((c^2 / (c^2 + n^2 + eps))^p, 0, 1) of two fp32 device tensors of one shape: like the reference
    it SQUARES its inputs, so they are magnitudes.  p = 0.5 takes a square root, any other p > 0 powf.  A complex input is
    refused.  -> fp32 device tensor, no autograd history."""
    if not p > 0:
        raise ValueError("compute_irm: p must be positive; got %r" % (p,))
    c, n = planes("compute_irm", clean_mag, noise_mag)
    return ops.mask_irm(c, n, p, eps)
