"""Mirror of signal_processing/haircell.py: the Meddis (1986) inner hair cell on device tensors (csrc/haircell.hip).

A (utterance, channel) is one chain of Euler steps in float64; the kernel keeps the reference's operation order and its three
clamps and fuses no multiply-add, so process / process_filterbank equal the reference fed the same fp32-valued input bit for
bit.  The steady state (q0, c0, w0) is computed on the host in Python floats exactly as the reference computes it.
process_to_frames does not store the firing-rate signal (8 bytes x B C L): a chain carries the sums of the two frames that
cover its sample and writes the means."""
import numpy as np
import torch

from .. import ops


class MeddisHairCell:
    """hc = MeddisHairCell(); ns = hc.process_to_frames(gfb.filter(wave))       # [C, L] / [B, C, L] fp32 -> [.., C, T] float64

    Methods take fp32 device tensors - what GammatoneFilterbank.filter returns - and return float64 device tensors without
    autograd history.  A host tensor is refused: there is no CPU fallback."""

    def __init__(self, sample_rate=8000):
        self.fs = sample_rate
        self.dt = 1.0 / sample_rate
        self.A = 5.0
        self.B = 300.0
        self.g = 2000.0
        self.y = 5.05
        self.l = 2500.0
        self.r = 6580.0
        self.x = 66.31
        self.h = 50000.0
        self.M = 1.0
        self._compute_steady_state()
        self._dev = {}

    def _compute_steady_state(self):
        k_ss = self.g * self.A / (self.A + self.B)
        self.q0 = self.M * self.y * k_ss / (self.l * k_ss + self.y * (self.l + self.r))
        self.c0 = self.q0 * k_ss / self.y
        self.w0 = self.c0 * self.r / self.x

    def _par(self, device):
        """the kernel's fp64 parameter vector, from the attributes as they are now"""
        vals = (self.A, self.B, self.y, self.l, self.r, self.x, self.h, self.M, self.dt, self.q0, self.c0, self.w0)
        key = (str(device),) + vals
        if key not in self._dev:
            self._dev = {key: torch.from_numpy(np.asarray(vals, dtype=np.float64)).to(device)}
        return self._dev[key]

    @staticmethod
    def _input(name, x, dims):
        if not torch.is_tensor(x):
            raise TypeError("%s: a device tensor is needed; got %s" % (name, type(x).__name__))
        if not x.is_cuda:
            raise RuntimeError("%s: the sincformer HIP path only runs on an MI355X device tensor; got a CPU tensor "
                               "(there is deliberately no CPU fallback)." % name)
        if x.dtype != torch.float32:
            raise TypeError("%s: an fp32 tensor is needed; got %s" % (name, x.dtype))
        if x.dim() not in dims or x.numel() == 0:
            raise ValueError("%s: input %s; %s is needed" % (name, tuple(x.shape), " or ".join(
                {1: "[L]", 2: "[C, L]", 3: "[B, C, L]"}[d] for d in dims)))
        return x.detach().contiguous()

    def process(self, signal):
        """[L] -> [L] float64: the firing rate h c[t] of one channel's signal"""
        x = self._input("MeddisHairCell.process", signal, (1,))
        return ops.haircell(x.reshape(1, -1), self._par(x.device))[0]

    def process_filterbank(self, filterbank_output):
        """[C, L] / [B, C, L] -> the same shape, float64: process of every row"""
        x = self._input("MeddisHairCell.process_filterbank", filterbank_output, (2, 3))
        return ops.haircell(x.reshape(-1, x.shape[-1]), self._par(x.device)).reshape(x.shape)

    def process_to_frames(self, filterbank_output, frame_size=160, hop_size=80, lengths=None):
        """[C, L] / [B, C, L] -> [C, T] / [B, C, T] float64, T = (L - frame_size) // hop_size + 1: the mean firing rate over each
        frame.  frame_size <= 2 hop_size (a sample lies in at most two frames).  With lengths (B sample counts, [B, C, L] only)
        utterance b has T_b frames and zeros from there on, and gets the bits it gets alone."""
        name = "MeddisHairCell.process_to_frames"
        frame, hop = int(frame_size), int(hop_size)
        if frame < 1 or hop < 1 or frame > 2 * hop:
            raise ValueError("%s: frame_size %r, hop_size %r; 1 <= frame_size <= 2 hop_size is needed" % (name, frame_size, hop_size))
        x = self._input(name, filterbank_output, (2, 3))
        if x.shape[-1] < frame:
            raise ValueError("%s: %d samples are shorter than one frame of %d" % (name, x.shape[-1], frame))
        two_d = x.dim() == 2
        x3 = x.reshape(1, *x.shape) if two_d else x
        if lengths is not None:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
            if two_d or host.size != x3.shape[0] or int(host.min()) < 1 or int(host.max()) > x3.shape[2]:
                raise ValueError("%s: lengths %r for input %s" % (name, host.tolist(), tuple(x.shape)))
            lengths = torch.from_numpy(host.astype(np.int32)).to(x.device)
        out = ops.haircell_frames(x3, self._par(x.device), frame, hop, lengths)
        return out[0] if two_d else out
