"""Mirror of signal_processing/gammatone.py: the 64-channel gammatone filterbank (paper Eq. 2-3) and its T-F analysis on
device tensors (csrc/gammatone.hip).

The filters are designed on the host in numpy float64 exactly as the reference designs them; the analysis runs on the device.
get_tf_magnitudes needs no FFT: for a frame f of w = min(frame_size, N) samples and even N, the sum of |rfft(f, N)|^2 over the
N/2 + 1 bins is (N sum f^2 + (sum f)^2 + (sum (-1)^t f)^2) / 2 and the one bin whose phase is read is two dot products, so a
(channel, frame) is five sums.  With hop_size * 2 == frame_size they are taken per hop-block inside the FIR kernel and a frame is
two neighbouring blocks (the second turned by exp(-2 pi i k hop / N)): the filtered signal is never stored.  Any other framing
stores it (filter) and takes the five sums per frame from it."""
import numpy as np
import torch

from .. import config, ops


def erb_bandwidth(cf):
    """Glasberg & Moore's equivalent rectangular bandwidth of a centre frequency in Hz"""
    return 24.7 * (4.37 * cf / 1000.0 + 1.0)


def erb_space(low_freq, high_freq, num_channels):
    """num_channels centre frequencies from low_freq to high_freq, equally spaced on the ERB-number scale"""
    q = 24.7 * 9.265
    lo = 9.265 * np.log(1 + low_freq / q)
    hi = 9.265 * np.log(1 + high_freq / q)
    return q * (np.exp(np.linspace(lo, hi, num_channels) / 9.265) - 1)


def gammatone_impulse_response(cf, fs, duration=0.05, order=4):
    """t^(order - 1) exp(-2 pi 1.019 ERB(cf) t) cos(2 pi cf t) on t = 0, 1/fs, .. < duration, scaled to unit energy"""
    t = np.arange(0, duration, 1.0 / fs)
    b = 2 * np.pi * erb_bandwidth(cf) * 1.019
    g = (t ** (order - 1)) * np.exp(-b * t) * np.cos(2 * np.pi * cf * t)
    return g / (np.sqrt(np.sum(g ** 2)) + 1e-10)


class GammatoneFilterbank:
    """gfb = GammatoneFilterbank(); magnitudes, phases = gfb.get_tf_magnitudes(wave)      # wave: fp32 device tensor [L] or [B, L]

    Methods take fp32 device tensors, 1-D or [B, L], and an optional lengths= (a sequence or tensor of B sample counts) for a
    zero-padded batch; results are fp32 device tensors without autograd history.  A host tensor is refused: there is no CPU
    fallback.  The kernels take at most 64 channels and 2048 taps."""

    def __init__(self, num_channels=None, freq_low=None, freq_high=None, sample_rate=None, filter_order=None):
        self.num_channels = num_channels or config.NUM_CHANNELS
        self.freq_low = freq_low or config.FREQ_LOW
        self.freq_high = freq_high or config.FREQ_HIGH
        self.sample_rate = sample_rate or config.SAMPLE_RATE
        self.filter_order = filter_order or config.FILTER_ORDER
        self.center_freqs = erb_space(self.freq_low, self.freq_high, self.num_channels)
        self.impulse_responses = [gammatone_impulse_response(cf, self.sample_rate, order=self.filter_order)
                                  for cf in self.center_freqs]
        self._dev = {}                                       # (what, device, ...) -> device tensor

    # ---- host-built operands, cached per device ----
    def cf_bins(self, fft_size):
        """the rfft bin whose phase get_tf_magnitudes reads, per channel"""
        return [min(int(cf * fft_size / self.sample_rate), fft_size // 2) for cf in self.center_freqs]

    def _taps(self, device):
        """[K, 64] fp32, tap-major: K = the tap count rounded up to a multiple of 8, columns from num_channels on zero"""
        key = ("taps", str(device))
        if key not in self._dev:
            n = len(self.impulse_responses[0])
            if self.num_channels > ops.GT_COLS or n > ops.GT_MAX_TAPS:
                raise ValueError("GammatoneFilterbank: %d channels x %d taps; the kernels take <= %d x %d" % (
                    self.num_channels, n, ops.GT_COLS, ops.GT_MAX_TAPS))
            h = np.zeros((-(-n // 8) * 8, ops.GT_COLS), dtype=np.float32)
            h[:n, :self.num_channels] = np.stack(self.impulse_responses, axis=1)
            self._dev[key] = torch.from_numpy(h).to(device)
        return self._dev[key]

    def _twiddles(self, device, n_t, fft_size):
        """[2, n_t, 64] fp32: cos, sin of 2 pi ((k_c t) mod N) / N in float64; the sine is exactly 0 at index 0 and N / 2"""
        key = ("tw", str(device), n_t, fft_size)
        if key not in self._dev:
            k = np.asarray(self.cf_bins(fft_size), dtype=np.int64)
            idx = (np.arange(n_t, dtype=np.int64)[:, None] * k[None, :]) % fft_size
            ang = 2.0 * np.pi * idx.astype(np.float64) / fft_size
            sin = np.sin(ang)
            sin[(idx == 0) | (2 * idx == fft_size)] = 0.0
            tw = np.zeros((2, n_t, ops.GT_COLS), dtype=np.float32)
            tw[0, :, :self.num_channels] = np.cos(ang)
            tw[1, :, :self.num_channels] = sin
            self._dev[key] = torch.from_numpy(tw).to(device)
        return self._dev[key]

    # ---- arguments ----
    def _signal(self, name, signal, lengths):
        """-> (sig [B, L] contiguous, lengths int32 device tensor or None, one_d)"""
        if not torch.is_tensor(signal):
            raise TypeError("%s: a device tensor is needed; got %s" % (name, type(signal).__name__))
        if not signal.is_cuda:
            raise RuntimeError("%s: the sincformer HIP path only runs on an MI355X device tensor; got a CPU tensor "
                               "(there is deliberately no CPU fallback)." % name)
        if signal.dtype != torch.float32:
            raise TypeError("%s: an fp32 tensor is needed; got %s" % (name, signal.dtype))
        if signal.dim() not in (1, 2) or signal.numel() == 0:
            raise ValueError("%s: signal %s; [L] or [B, L] is needed" % (name, tuple(signal.shape)))
        one_d = signal.dim() == 1
        sig = signal.detach().reshape(1, -1) if one_d else signal.detach()
        sig = sig.contiguous()
        if lengths is not None:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
            if host.size != sig.shape[0] or int(host.min()) < 1 or int(host.max()) > sig.shape[1]:
                raise ValueError("%s: lengths %r for %d signals of %d samples" % (name, host.tolist(), sig.shape[0], sig.shape[1]))
            lengths = torch.from_numpy(host.astype(np.int32)).to(sig.device)
        return sig, lengths, one_d

    # ---- the reference's three methods ----
    def filter(self, signal, lengths=None):
        """(C, L) / [B, C, L]: row i = (signal * impulse_responses[i])[:L], the causal convolution (Eq. 3); 0 from lengths[b] on"""
        sig, lengths, one_d = self._signal("GammatoneFilterbank.filter", signal, lengths)
        y = ops.gammatone_fir(sig, self._taps(sig.device), self.num_channels, lengths)
        return y[0] if one_d else y

    def _framing(self, name, L, frame_size, hop_size):
        frame_size = frame_size or config.FRAME_SIZE
        hop_size = hop_size or config.HOP_SIZE
        if frame_size < 1 or hop_size < 1:
            raise ValueError("%s: frame_size %r, hop_size %r" % (name, frame_size, hop_size))
        if L < frame_size:
            raise ValueError("%s: %d samples are shorter than one frame of %d" % (name, L, frame_size))
        return int(frame_size), int(hop_size), (L - frame_size) // hop_size + 1

    def filter_to_frames(self, signal, frame_size=None, hop_size=None, lengths=None):
        """(C, T, frame_size) / [B, C, T, frame_size]: frame n = filter(signal)[.., n hop : n hop + frame_size], a strided copy"""
        sig, lengths, one_d = self._signal("GammatoneFilterbank.filter_to_frames", signal, lengths)
        frame, hop, T = self._framing("GammatoneFilterbank.filter_to_frames", sig.shape[1], frame_size, hop_size)
        y = ops.gammatone_fir(sig, self._taps(sig.device), self.num_channels, lengths)
        frames = y.unfold(2, frame, hop).contiguous()
        if lengths is not None:                               # frames that end behind the utterance are 0
            Tb = torch.clamp((lengths.long() - frame) // hop + 1, min=0)
            frames *= (torch.arange(T, device=y.device)[None, :] < Tb[:, None])[:, None, :, None]
        return frames[0] if one_d else frames

    def get_tf_magnitudes(self, signal, frame_size=None, hop_size=None, fft_size=None, want_bins=False, lengths=None):
        """(magnitudes, phases), each (C, T) / [B, C, T], T = (L - frame_size) // hop_size + 1: the sum of |rfft(frame, N)|^2 over
        the bins and the angle of bin min(int(cf N / fs), N // 2); want_bins=True adds that bin's real and imaginary part.
        With lengths, utterance b has its own T_b frames and zeros from there on, and gets the bits it gets alone."""
        name = "GammatoneFilterbank.get_tf_magnitudes"
        sig, lengths, one_d = self._signal(name, signal, lengths)
        L = sig.shape[1]
        frame, hop, T = self._framing(name, L, frame_size, hop_size)
        N = int(fft_size or config.FFT_SIZE)
        if N < 2 or N % 2:
            raise ValueError("%s: fft_size %d; an even size is needed (the Parseval form of the bin sum)" % (name, N))
        dev, C = sig.device, self.num_channels
        taps = self._taps(dev)
        fused = hop * 2 == frame and hop % 2 == 0 and N >= frame and ops.gammatone_tf_fits(taps.shape[0], hop)
        if fused and ops.switch("gammatone_fused"):
            partial = ops.gammatone_tf(sig, taps, self._twiddles(dev, hop, N), C, hop, lengths)
            key = ("rot", str(dev), hop, N)
            if key not in self._dev:
                self._dev[key] = self._twiddles(dev, hop + 1, N)[:, hop, :].contiguous()
            out = ops.gammatone_tf_finish(partial, self._dev[key], T, L, frame, hop, N, True, lengths, want_bins)
        else:
            w = min(frame, N)                                 # np.fft.rfft crops a longer frame to N
            y = ops.gammatone_fir(sig, taps, C, lengths)
            partial = ops.gammatone_moments(y, self._twiddles(dev, w, N), T, w, frame, hop, lengths)
            out = ops.gammatone_tf_finish(partial, None, T, L, frame, hop, N, False, lengths, want_bins)
        return tuple(o[0] for o in out) if one_d else out

    def block_sums(self, signal, hop_size=None, fft_size=None, lengths=None):
        """[B, L // hop, C, 5] (or without B): {sum y^2, sum y, sum (-1)^t y, sum y cos, sum y sin} of every whole hop-block of
        the filtered signal with the block-local t: what the fused route of get_tf_magnitudes combines (for inspection and tests)"""
        sig, lengths, one_d = self._signal("GammatoneFilterbank.block_sums", signal, lengths)
        hop, N = int(hop_size or config.HOP_SIZE), int(fft_size or config.FFT_SIZE)
        taps = self._taps(sig.device)
        if N % 2 or not ops.gammatone_tf_fits(taps.shape[0], hop) or sig.shape[1] < hop:
            raise ValueError("GammatoneFilterbank.block_sums: hop %d, fft_size %d, %d samples are not taken by the fused kernel" % (
                hop, N, sig.shape[1]))
        p = ops.gammatone_tf(sig, taps, self._twiddles(sig.device, hop, N), self.num_channels, hop, lengths)
        return p[0] if one_d else p
