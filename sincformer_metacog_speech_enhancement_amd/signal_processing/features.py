"""Mirror of signal_processing/features.py: the DNN's front end [AMS 15 | RASTA-PLP 13 | MFCC 13 | GFCC 13] per frame of 160
samples at hop 80, and its context, on device tensors (csrc/features.hip, csrc/framed_gemm.hip, csrc/gammatone.hip).

Everything built on the host - the symmetric Hamming windows, the mel matrix [64, 257], the bark matrix [21, 129], the
equal-loudness vector, the orthonormal DCT-II rows - is numpy float64 and needs no scipy.  On the device:

  MFCC       pre-emphasis, Hamming(160) and the 512-point DFT are ONE operand [161, 514] of the exact-fp32 framed GEMM: row j + 1
             holds w[j] e(j) - 0.97 w[j + 1] e(j + 1), so a frame reads its 160 samples and the one before them, and sample -1 of
             an utterance reads as 0 (pre[0] = x[0]).  Then power -> mel -> log(. + 1e-10) -> DCT in the cepstral kernel.
  RASTA-PLP  Hamming(160) and the 256-point DFT are 258 more columns of the same operand (one launch, the signal is read once);
             power -> bark -> log in the cepstral kernel, then the RASTA kernel: the filter along the utterance's own frames, exp,
             equal loudness, cube root, mean, DCT in fp64, one vector per utterance on all of its rows.
  GFCC       gfb.filter is never stored: the window of fs // 100 samples centred on n hop + frame / 2 is two neighbouring hop-blocks
             of sfm_gammatone_tf's block sums (sum y^2; 8 kHz: blocks 2 n + 1, 2 n + 2 of 40; 16 kHz: blocks n, n + 1 of 80); mean,
             signed cube root and DCT in the cepstral kernel.
  AMS        in extract_frame_features the reference hands extract_ams 640 samples, 80 after its decimation by 8 - fewer than one
             128-sample segment - so its loop ends before the first segment: the 15 columns are exactly 0 for every input and both
             sample rates.  They are written as zeros and nothing is launched.  Stand-alone extract_ams on a longer signal is
             mirrored.

All frame constants (160, 80, 256, 512) are config values independent of fs; only the filterbanks and fs // 100 follow fs."""
import numpy as np
import torch

from .. import config, ops
from .gammatone import GammatoneFilterbank

NUM_BARK_FILTERS = 21
PREEMPHASIS = 0.97


# ---- host helpers (numpy float64) ----
def hz_to_bark(f):
    """frequency in Hz -> Bark"""
    return 6.0 * np.arcsinh(f / 600.0)


def bark_to_hz(z):
    """Bark -> frequency in Hz"""
    return 600.0 * np.sinh(z / 6.0)


def hz_to_mel(f):
    """frequency in Hz -> mel"""
    return 2595.0 * np.log10(1 + f / 700.0)


def mel_to_hz(m):
    """mel -> frequency in Hz"""
    return 700.0 * (10 ** (m / 2595.0) - 1)


def hamming(n):
    """the symmetric Hamming window 0.54 - 0.46 cos(2 pi t / (n - 1)), evaluated as 0.54 + 0.46 cos on linspace(-pi, pi, n)"""
    if n == 1:
        return np.ones(1)
    return 0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, n))


def mel_filterbank(num_filters, fft_size, fs):
    """[num_filters, fft_size // 2 + 1]: triangles between the bins floor((fft_size + 1) hz / fs) of num_filters + 2 mel-spaced
    points from 0 to fs / 2"""
    hz_points = mel_to_hz(np.linspace(hz_to_mel(0), hz_to_mel(fs / 2), num_filters + 2))
    bins = np.floor((fft_size + 1) * hz_points / fs).astype(int)
    fb = np.zeros((num_filters, fft_size // 2 + 1))
    for i in range(num_filters):
        for j in range(bins[i], min(bins[i + 1], fb.shape[1])):
            fb[i, j] = (j - bins[i]) / (bins[i + 1] - bins[i] + 1e-10)
        for j in range(bins[i + 1], min(bins[i + 2], fb.shape[1])):
            fb[i, j] = (bins[i + 2] - j) / (bins[i + 2] - bins[i + 1] + 1e-10)
    return fb


def _triangles(edges, freq_bins):
    """[len(edges) - 2, len(freq_bins)]: rising on [lo, mid], falling on (mid, hi], slopes over (width + 1e-10)"""
    fb = np.zeros((len(edges) - 2, len(freq_bins)))
    for i in range(len(edges) - 2):
        lo, mid, hi = edges[i], edges[i + 1], edges[i + 2]
        rise = (freq_bins >= lo) & (freq_bins <= mid)
        fall = (freq_bins > mid) & (freq_bins <= hi)
        fb[i, rise] = (freq_bins[rise] - lo) / (mid - lo + 1e-10)
        fb[i, fall] = (hi - freq_bins[fall]) / (hi - mid + 1e-10)
    return fb


def bark_filterbank(fs, fft_size=None, num_filters=NUM_BARK_FILTERS):
    """(matrix [num_filters, fft_size // 2 + 1], equal-loudness vector [num_filters]) of extract_rasta_plp"""
    fft_size = fft_size or config.FFT_SIZE
    centers = np.linspace(hz_to_bark(0), hz_to_bark(fs / 2), num_filters + 2)
    fb = _triangles(bark_to_hz(centers), np.arange(fft_size // 2 + 1) * fs / fft_size)
    eql = np.ones(num_filters)
    for i in range(num_filters):
        f = bark_to_hz(centers[i + 1])
        eql[i] = f ** 2 / (f ** 2 + 1.6e5)
    return fb, eql


def ams_filterbank(fs, num_bands=None):
    """[num_bands, AMS_FFT_SIZE // 2 + 1]: extract_ams's triangles between 15.6 and 400 Hz on the bins of the decimated rate fs / 8"""
    num_bands = num_bands or config.AMS_NUM_BANDS
    freq_bins = np.arange(config.AMS_FFT_SIZE // 2 + 1) * (fs / 8) / config.AMS_FFT_SIZE
    return _triangles(np.linspace(15.6, 400.0, num_bands + 2), freq_bins)


def dct_rows(num_coeffs, m):
    """the first num_coeffs rows [num_coeffs, m] of the orthonormal DCT-II: sqrt(2 / m) cos(pi k (2 n + 1) / (2 m)), row 0 over sqrt 2"""
    k = np.arange(num_coeffs, dtype=np.int64)[:, None]
    n = np.arange(m, dtype=np.int64)[None, :]
    rows = 2.0 * np.cos(np.pi * ((k * (2 * n + 1)) % (4 * m)).astype(np.float64) / (2.0 * m)) * np.sqrt(1.0 / (2.0 * m))
    rows[0] = 2.0 * np.sqrt(1.0 / (4.0 * m))
    return rows


def dft_operand(window, fft_size, preemphasis=0.0, stop=None):
    """[len(window) + 1, 2 (fft_size // 2 + 1)] float64, columns cos | sin: the operand whose product with the samples
    x[s - 1 .. s + len(window)) is the rfft of window * pre[s ..], pre[t] = x[t] - preemphasis x[t - 1]; stop: pre[t] = 0 from
    frame sample `stop` on (a signal of `stop` samples that is padded AFTER its pre-emphasis, as extract_mfcc pads)"""
    n = len(window)
    t = np.arange(n, dtype=np.int64)[:, None]
    k = np.arange(fft_size // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((t * k) % fft_size).astype(np.float64) / fft_size
    e = np.concatenate([np.cos(ang), np.sin(ang)], axis=1) * window[:, None]
    op = np.zeros((n + 1, e.shape[1]))
    op[1:] = e
    stop = n if stop is None else stop
    op[:stop] -= preemphasis * e[:stop]
    return op


_DEV = {}                                                    # (what, device, ...) -> device tensor


def _cached(key, make):
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def _f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _f64(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _signal(name, signal, lengths, min_len):
    """-> (sig [B, L >= min_len] contiguous fp32, lengths int32 device tensor (>= min_len) or None, one_d).  A signal shorter than
    min_len is zero-padded to it, as the reference pads; with lengths, samples behind a short utterance's end are zeroed first."""
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
    host = None
    if lengths is not None:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
        if host.size != sig.shape[0] or int(host.min()) < 1 or int(host.max()) > sig.shape[1]:
            raise ValueError("%s: lengths %r for %d signals of %d samples" % (name, host.tolist(), sig.shape[0], sig.shape[1]))
    if sig.shape[1] < min_len:
        sig = torch.nn.functional.pad(sig, (0, min_len - sig.shape[1]))
    if host is not None and int(host.min()) < min_len:        # the padding of a short utterance inside a longer buffer
        keep = torch.arange(sig.shape[1], device=sig.device)[None, :] < torch.from_numpy(host).to(sig.device)[:, None]
        sig = sig * keep
        host = np.maximum(host, min_len)
    dev_len = None if host is None else torch.from_numpy(host.astype(np.int32)).to(sig.device)
    return sig.contiguous(), dev_len, one_d


def _frame_count(L):
    return (L - config.FRAME_SIZE) // config.HOP_SIZE + 1


def _spectra_operand(device, stop=None):
    """[192, 832] fp32 operand of the framed GEMM: K = 161 rows, columns [MFCC cos 257 | sin 257 | RASTA cos 129 | sin 129]"""
    def make():
        w = hamming(config.FRAME_SIZE)
        op = np.concatenate([dft_operand(w, config.MFCC_FFT_SIZE, PREEMPHASIS, stop), dft_operand(w, config.FFT_SIZE)], axis=1)
        return ops.pack_f32_matrix(_f32(op, device))
    return _cached(("spectra", str(device), stop), make)


def _spectra(sig, stop=None):
    """sig [B, L] -> [B, T, 772]: both analysis DFTs of every frame in one launch of the exact-fp32 framed GEMM"""
    B, L = sig.shape
    T = _frame_count(L)
    Fm, Fr = config.MFCC_FFT_SIZE // 2 + 1, config.FFT_SIZE // 2 + 1
    N = 2 * (Fm + Fr)
    spec = torch.empty(B, T, N, device=sig.device, dtype=torch.float32)
    ops.framed_gemm(sig, _spectra_operand(sig.device, stop), spec, B=B, M=T, Ls=L, sig_batch_stride=L, hop=config.HOP_SIZE, padl=1,
                    K=config.FRAME_SIZE + 1, N=N, o_batch_stride=T * N, ldm=N, ldn=1, mode=0)
    return spec


def _framing(L):
    return dict(L=L, frame=config.FRAME_SIZE, hop=config.HOP_SIZE)


def _mfcc_into(out, col, spec, fs, num_coeffs, lengths, L):
    dev = out.device
    Fm = config.MFCC_FFT_SIZE // 2 + 1
    mel = _cached(("mel", str(dev), fs), lambda: _f32(mel_filterbank(config.MFCC_NUM_FILTERS, config.MFCC_FFT_SIZE, fs), dev))
    dct = _cached(("dct", str(dev), num_coeffs, config.MFCC_NUM_FILTERS), lambda: _f32(dct_rows(num_coeffs, config.MFCC_NUM_FILTERS), dev))
    B, T = out.shape[:2]
    ops.cepstral(spec[:, :, :2 * Fm], mel, dct, out, col, B=B, T=T, in_mode=ops.CEP_POWER, F=Fm, im_off=Fm, compress=ops.CEP_LOG,
                 lengths=lengths, **_framing(L))


def _rasta_into(out, col, spec, fs, num_coeffs, lengths, L):
    dev = out.device
    Fm, Fr = config.MFCC_FFT_SIZE // 2 + 1, config.FFT_SIZE // 2 + 1
    bark = _cached(("bark", str(dev), fs), lambda: _f32(bark_filterbank(fs)[0], dev))
    eql = _cached(("eql", str(dev), fs), lambda: _f64(bark_filterbank(fs)[1], dev))
    dct = _cached(("dct64", str(dev), num_coeffs, NUM_BARK_FILTERS), lambda: _f64(dct_rows(num_coeffs, NUM_BARK_FILTERS), dev))
    B, T = out.shape[:2]
    logb = torch.empty(B, T, NUM_BARK_FILTERS, device=dev, dtype=torch.float32)
    ops.cepstral(spec[:, :, 2 * Fm:], bark, None, logb, 0, B=B, T=T, in_mode=ops.CEP_POWER, F=Fr, im_off=Fr, compress=ops.CEP_LOG,
                 lengths=lengths, **_framing(L))
    ops.rasta(logb, eql, dct, out, col, lengths=lengths, **_framing(L))


def gfcc_blocks(fs, gfb, centred):
    """(block hop, bmul, badd, window) of the GFCC window in sfm_gammatone_tf's hop-blocks: fs // 100 samples centred on
    n hop + frame / 2 (extract_frame_features) or the block [n w, (n + 1) w) (extract_gfcc); ValueError when the window is not made
    of two whole blocks that the fused kernel takes"""
    w = fs // config.GFCC_DECIMATE_RATE
    h = w // 2
    taps = -(-len(gfb.impulse_responses[0]) // 8) * 8
    ok = w >= 4 and w == 2 * h and h % 2 == 0 and ops.gammatone_tf_fits(taps, h) and gfb.num_channels <= ops.FE_MAX_FILTERS
    if centred:
        ok = ok and config.HOP_SIZE % h == 0 and h <= config.FRAME_SIZE // 2 and (config.FRAME_SIZE // 2 - h) % h == 0
    if not ok:
        raise ValueError("GFCC at fs %d: a window of %d samples is not made of whole hop-blocks that the fused gammatone kernel takes "
                         "(8000 and 16000 are supported)" % (fs, w))
    return (h, config.HOP_SIZE // h, (config.FRAME_SIZE // 2 - h) // h, w) if centred else (h, 2, 0, w)


def _gfcc_into(out, col, sig, gfb, blocks, num_coeffs, lengths, L, frame, hop):
    dev = out.device
    h, bmul, badd, w = blocks
    C = gfb.num_channels
    dct = _cached(("dct", str(dev), num_coeffs, C), lambda: _f32(dct_rows(num_coeffs, C), dev))
    partial = ops.gammatone_tf(sig, gfb._taps(dev), gfb._twiddles(dev, h, config.FFT_SIZE), C, h, lengths)
    B, T = out.shape[:2]
    ops.cepstral(partial, None, dct, out, col, B=B, T=T, L=L, frame=frame, hop=hop, in_mode=ops.CEP_BLOCKS, F=C,
                 compress=ops.CEP_CBRT, bmul=bmul, badd=badd, window=float(w), lengths=lengths)


# ---- the stand-alone extractors: per-utterance vectors ----
def extract_mfcc(signal, fs=None, num_coeffs=None, lengths=None):
    """[num_coeffs] / [B, num_coeffs]: the mean over an utterance's frames of its MFCC rows"""
    fs, nc = fs or config.SAMPLE_RATE, num_coeffs or config.MFCC_NUM_COEFF
    raw_len = signal.shape[-1] if torch.is_tensor(signal) and signal.dim() else 0
    if lengths is not None:
        if int(np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).min()) < config.FRAME_SIZE:
            raise ValueError("extract_mfcc: with lengths, an utterance shorter than one frame of %d is not taken (the "
                             "reference pads it after its pre-emphasis, which needs an operand per length)" % config.FRAME_SIZE)
    sig, lengths, one_d = _signal("extract_mfcc", signal, lengths, config.FRAME_SIZE)
    B, L = sig.shape
    # the reference pads a short signal AFTER its pre-emphasis here (pre[len] = 0, not -0.97 x[len - 1]): an operand of its own
    stop = raw_len if raw_len < config.FRAME_SIZE else None
    rows = torch.zeros(B, _frame_count(L), nc, device=sig.device, dtype=torch.float32)
    _mfcc_into(rows, 0, _spectra(sig, stop), fs, nc, lengths, L)
    out = ops.rows_mean(rows, 0, nc, lengths=lengths, **_framing(L))
    return out[0] if one_d else out


def extract_rasta_plp(signal, fs=None, num_coeffs=None, lengths=None):
    """[num_coeffs] / [B, num_coeffs]: the utterance's RASTA-PLP vector"""
    fs, nc = fs or config.SAMPLE_RATE, num_coeffs or config.RASTA_NUM_COEFF
    sig, lengths, one_d = _signal("extract_rasta_plp", signal, lengths, config.FRAME_SIZE)
    B, L = sig.shape
    rows = torch.zeros(B, _frame_count(L), nc, device=sig.device, dtype=torch.float32)
    _rasta_into(rows, 0, _spectra(sig), fs, nc, lengths, L)
    out = rows[:, 0].contiguous()
    return out[0] if one_d else out


def extract_gfcc(signal, fs=None, num_coeffs=None, gfb=None, lengths=None):
    """[num_coeffs] / [B, num_coeffs]: the mean over the len // (fs // 100) whole blocks of fs // 100 samples of their GFCC rows
    (zeros for a signal shorter than one block)"""
    fs, nc = fs or config.SAMPLE_RATE, num_coeffs or config.GFCC_NUM_COEFF
    gfb = gfb or GammatoneFilterbank(sample_rate=fs)
    blocks = gfcc_blocks(fs, gfb, centred=False)
    w = blocks[3]
    sig, lengths, one_d = _signal("extract_gfcc", signal, lengths, 1)
    B, L = sig.shape
    if L < w:
        out = torch.zeros(B, nc, device=sig.device, dtype=torch.float32)
    else:
        rows = torch.zeros(B, L // w, nc, device=sig.device, dtype=torch.float32)
        _gfcc_into(rows, 0, sig, gfb, blocks, nc, lengths, L, w, w)
        out = ops.rows_mean(rows, 0, nc, L=L, frame=w, hop=w, lengths=lengths)
    return out[0] if one_d else out


def extract_ams(signal, fs=None, num_bands=None):
    """[num_bands] / [B, num_bands]: |x|[::8], segments of 128 at hop 64, Hamming, 256-point magnitude, the triangles, summed over
    the segments and divided by num_segs = max(1, (len - 128) // 64 + 1); zeros when the decimated signal is shorter than a segment"""
    fs, nb = fs or config.SAMPLE_RATE, num_bands or config.AMS_NUM_BANDS
    sig, _, one_d = _signal("extract_ams", signal, None, 1)
    dec = sig.abs()[:, ::8].contiguous()
    B, Ld = dec.shape
    seg, hop, N = config.AMS_SEGMENTS, config.AMS_SEGMENTS - config.AMS_OVERLAP, config.AMS_FFT_SIZE
    if Ld < seg:
        out = torch.zeros(B, nb, device=sig.device, dtype=torch.float32)
    else:
        S, F = (Ld - seg) // hop + 1, N // 2 + 1
        dev = sig.device
        op = _cached(("ams_op", str(dev)), lambda: ops.pack_f32_matrix(_f32(dft_operand(hamming(seg), N)[1:], dev)))
        tri = _cached(("ams_tri", str(dev), fs, nb), lambda: _f32(ams_filterbank(fs, nb), dev))
        spec = torch.empty(B, S, 2 * F, device=dev, dtype=torch.float32)
        ops.framed_gemm(dec, op, spec, B=B, M=S, Ls=Ld, sig_batch_stride=Ld, hop=hop, padl=0, K=seg, N=2 * F,
                        o_batch_stride=S * 2 * F, ldm=2 * F, ldn=1, mode=0)
        rows = torch.empty(B, S, nb, device=dev, dtype=torch.float32)
        ops.cepstral(spec, tri, None, rows, 0, B=B, T=S, L=Ld, frame=seg, hop=hop, in_mode=ops.CEP_MAGNITUDE, F=F, im_off=F,
                     compress=ops.CEP_NONE)
        out = ops.rows_mean(rows, 0, nb, L=Ld, frame=seg, hop=hop, den=S)
    return out[0] if one_d else out


class FeatureExtractor:
    """fe = FeatureExtractor(); x = fe.add_context(fe.extract_frame_features(wave))       # wave: fp32 device tensor [L] or [B, L]

    Methods take fp32 device tensors, 1-D or [B, L], and an optional lengths= for a zero-padded batch; results are fp32 device
    tensors without autograd history.  A host tensor is refused: there is no CPU fallback.  fs 8000 and 16000 are supported."""

    def __init__(self, fs=None):
        self.fs = fs or config.SAMPLE_RATE
        self.gfb = GammatoneFilterbank(sample_rate=self.fs)
        self.context = config.CONTEXT_FRAMES
        self._blocks = gfcc_blocks(self.fs, self.gfb, centred=True)

    def extract_frame_features(self, signal, lengths=None):
        """[T, 54] / [B, T, 54], T = (max(L, 160) - 160) // 80 + 1: [AMS (zeros) | RASTA-PLP | MFCC | GFCC] per frame.  With lengths,
        utterance b has its own T_b frames and its own RASTA mean, zeros from T_b on, and gets the bits it gets alone."""
        sig, lengths, one_d = _signal("FeatureExtractor.extract_frame_features", signal, lengths, config.FRAME_SIZE)
        B, L = sig.shape
        a, r, m = config.AMS_NUM_BANDS, config.RASTA_NUM_COEFF, config.MFCC_NUM_COEFF
        out = torch.zeros(B, _frame_count(L), self.raw_feature_dim, device=sig.device, dtype=torch.float32)
        spec = _spectra(sig)
        _rasta_into(out, a, spec, self.fs, r, lengths, L)
        _mfcc_into(out, a + r, spec, self.fs, m, lengths, L)
        _gfcc_into(out, a + r + m, sig, self.gfb, self._blocks, config.GFCC_NUM_COEFF, lengths, L, config.FRAME_SIZE, config.HOP_SIZE)
        return out[0] if one_d else out

    def add_context(self, features, feat_mean=None, feat_std=None, lengths=None):
        """[T, D] / [B, T, D] -> [.., T, D (2 context + 1)]: row n = rows clamp(n - context .. n + context, 0, T_b - 1) flattened.
        With feat_mean and feat_std (the Dataset's, [D (2 context + 1)]) the same launch applies nan / inf -> 0, (f - mean) / std and
        the clip to +-10, in that order.  lengths: frame counts T_b of a zero-padded batch; rows from T_b on are 0."""
        name = "FeatureExtractor.add_context"
        if not torch.is_tensor(features):
            raise TypeError("%s: a device tensor is needed; got %s" % (name, type(features).__name__))
        if not features.is_cuda:
            raise RuntimeError("%s: the sincformer HIP path only runs on an MI355X device tensor; got a CPU tensor "
                               "(there is deliberately no CPU fallback)." % name)
        if features.dtype != torch.float32 or features.dim() not in (2, 3) or features.numel() == 0 or features.shape[-1] % 2:
            raise ValueError("%s: features %s %s; fp32 [T, D] or [B, T, D] with an even D is needed" % (name, features.dtype,
                                                                                                         tuple(features.shape)))
        if (feat_mean is None) != (feat_std is None):
            raise ValueError("%s: feat_mean and feat_std go together" % name)
        two_d = features.dim() == 2
        f = features.detach().reshape(1, *features.shape) if two_d else features.detach()
        f = f.contiguous()
        B, T, D = f.shape
        W = D * (2 * self.context + 1)
        stats = []
        for s in (feat_mean, feat_std):
            if s is not None:
                s = torch.as_tensor(np.asarray(s, dtype=np.float32) if not torch.is_tensor(s) else s).to(f.device, torch.float32).reshape(-1)
                if s.numel() != W:
                    raise ValueError("%s: statistics of %d values for rows of %d" % (name, s.numel(), W))
                stats.append(s.contiguous())
        dev_len = None
        if lengths is not None:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
            if host.size != B or int(host.min()) < 1 or int(host.max()) > T:
                raise ValueError("%s: frame counts %r for %d utterances of %d frames" % (name, host.tolist(), B, T))
            dev_len = torch.from_numpy(host.astype(np.int32)).to(f.device)
        # the kernel's framing in units of rows: frame = hop = 1, so that T_b = lengths[b]
        out = ops.feature_context(f, self.context, L=T, frame=1, hop=1, mean=stats[0] if stats else None,
                                  std=stats[1] if stats else None, clip=10.0, lengths=dev_len)
        return out[0] if two_d else out

    @property
    def raw_feature_dim(self):
        return config.AMS_NUM_BANDS + config.RASTA_NUM_COEFF + config.MFCC_NUM_COEFF + config.GFCC_NUM_COEFF

    @property
    def feature_dim(self):
        return self.raw_feature_dim * (2 * self.context + 1)
