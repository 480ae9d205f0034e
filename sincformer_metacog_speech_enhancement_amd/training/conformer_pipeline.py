"""Host-side mirror of the model / STFT / objective part of training/conformer_pipeline.py
(si_snr_loss :52, MultiResolutionSTFTLoss :74, batch_stft :196, batch_istft :205, SpeechEnhancer :218-301,
ConformerPipeline._compute_loss :539, _save_best :611, save_model :618, load_model :628, enhance_signal :653) and the
north-star agent composition (EnhancementPath; SURVEY.md §3.3 with the glue of DESIGN.md), and of what its data set does
to a batch (_add_noise_at_snr :142, the assignment of WaveformDataset :162-171) as device passes: mix_at_snr, mix_batch,
curriculum_batch; WaveformDataset :153-189 as WaveformSet, a waveform set kept on the device, and train :403-484 with its warm-up
and cosine schedule (WarmupCosineRule).
The file search, audio loading and resampling of the reference (prepare_data) are out of scope.
"""
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from .. import config, functional as Fn, ops
from .._hostmod import HipModule
from ..models.conformer import ConformerBlock
from ..agents.perception import PerceptionAgent
from ..agents.cpea import CorrelationPhaseEstimationAgent
from ..agents.msa import MaskSynthesisAgent
from ..agents.memory import EpisodicMemory


def batch_stft(waveform, fft_size, hop_size, frame_size):
    """training/conformer_pipeline.py:196-202 -> (real, imag) each [B, T, fft_size/2+1] fp32
    (contiguous; the reference returns transposed views of [B, F, T])."""
    if not waveform.is_cuda:
        raise RuntimeError("batch_stft: HIP path needs a device tensor (no CPU fallback)")
    return Fn.stft(waveform.float(), fft_size, hop_size, frame_size)


def batch_istft(stft_real, stft_imag, fft_size, hop_size, frame_size, length):
    """training/conformer_pipeline.py:205-211 -> [B, length] fp32."""
    if not stft_real.is_cuda:
        raise RuntimeError("batch_istft: HIP path needs a device tensor (no CPU fallback)")
    return Fn.istft(stft_real.float(), stft_imag.float(), length, fft_size, hop_size, frame_size)


# ---------------------------------------------------------------------------------------------------------------------------
# Curriculum batches: the SNR mix (:142-150, assigned as WaveformDataset does :162-171) and the oracle mask targets of masks/,
# made where the batch is consumed (csrc/masks.hip).  Clean utterances and the noise bank go to the device once.
# ---------------------------------------------------------------------------------------------------------------------------
class NoiseBank:
    """A list of 1-D fp32 device tensors as ONE concatenated buffer plus an int32 offset table [count + 1]"""

    def __init__(self, signals):
        signals = list(signals)
        if not signals:
            raise ValueError("noise bank: at least one noise signal is needed")
        for s in signals:
            if not torch.is_tensor(s) or not s.is_cuda:
                raise RuntimeError("noise bank: the HIP path needs device tensors (no CPU fallback); got a CPU tensor")
            if s.dim() != 1 or s.numel() == 0:
                raise ValueError("noise bank: 1-D non-empty signals are needed; got shape %s" % (tuple(s.shape),))
        sizes = [s.numel() for s in signals]
        if sum(sizes) > 2 ** 31 - 1:
            raise ValueError("noise bank: %d samples; the offset table is int32" % sum(sizes))
        self.count = len(signals)
        self.buffer = torch.cat([s.detach().float() for s in signals]).contiguous()
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=self.buffer.device)


_banks = {}


def noise_bank(signals):
    """the NoiseBank of a list of device tensors, built once per list content (storage, length and version of every entry)"""
    if isinstance(signals, NoiseBank):
        return signals
    signals = list(signals)
    key = tuple((s.data_ptr(), s.numel(), s._version, str(s.device)) if torch.is_tensor(s) else id(s) for s in signals)
    hit = _banks.get(key)
    if hit is None:
        if len(_banks) >= 8:
            _banks.clear()
        hit = _banks[key] = (NoiseBank(signals), signals)        # (the list is kept: a freed entry's address cannot come back)
    return hit[0]


def _mix_args(name, clean, bank, noise_ids, snr_db, lengths):
    if not torch.is_tensor(clean) or not clean.is_cuda:
        raise RuntimeError("%s: the HIP path needs device tensors (no CPU fallback); got a CPU tensor" % name)
    if clean.dim() != 2 or clean.numel() == 0:
        raise ValueError("%s: clean [B, L] is needed; got shape %s" % (name, tuple(clean.shape)))
    clean = clean.detach().float().contiguous()
    B, L = clean.shape
    dev = clean.device

    def column(v, dtype, what, lo=None, hi=None):
        if torch.is_tensor(v) and v.is_cuda:
            t = v.detach().to(dtype).contiguous()                # (a device column is trusted: the kernels clamp what they index with)
        else:
            a = np.asarray(v.cpu() if torch.is_tensor(v) else v).reshape(-1)
            if lo is not None and a.size and (a.min() < lo or a.max() > hi):
                raise ValueError("%s: %s outside %d..%d" % (name, what, lo, hi))
            t = torch.as_tensor(a).to(dtype).to(dev)
        if t.shape != (B,):
            raise ValueError("%s: %s must have one entry per utterance (%d); got shape %s" % (name, what, B, tuple(t.shape)))
        return t
    ids = column(noise_ids, torch.int32, "noise_ids", 0, bank.count - 1)
    snr = column(snr_db, torch.float32, "snr_db")
    lens = None if lengths is None else column(lengths, torch.int32, "lengths", 1, L)
    return clean, ids, snr, lens


def mix_at_snr(clean, noise_bank_, noise_ids, snr_db, lengths=None):
    """_add_noise_at_snr (:142-150) over a batch.  clean [B, L] (zero from lengths[i] on, as the reference pads), noise_bank_ a
    list of 1-D device tensors (or a NoiseBank), noise_ids [B], snr_db [B], lengths [B] or None (= L) -> (noisy [B, L], scale [B]).
    Per utterance: the noise is tiled when shorter (sample j reads noise[j mod Ln]) and cut when longer; the powers are means
    over the utterance's own lengths[i] samples plus 1e-10 each, summed in fp64 in a fixed order (no atomics: the same bits
    from run to run); scale = sqrt(Pc / (Pn 10^(snr / 10))); noisy = clean + scale * noise, 0 at and beyond lengths[i]."""
    bank = noise_bank(noise_bank_)
    clean, ids, snr, lens = _mix_args("mix_at_snr", clean, bank, noise_ids, snr_db, lengths)
    scale = ops.mix_scale(clean, bank.buffer, bank.offsets, ids, snr, lens)
    noisy, _ = ops.mix_apply(clean, bank.buffer, bank.offsets, ids, scale, lens)
    return noisy, scale


def _add_noise_at_snr(clean, noise, snr_db):
    """training/conformer_pipeline.py:142-150 for one utterance: 1-D device tensors -> the noisy utterance (mix_at_snr)"""
    return mix_at_snr(clean.reshape(1, -1), [noise.reshape(-1)], [0], [float(snr_db)])[0][0]


def mix_assignment(count, n_noise, snr_levels, first_index=0):
    """WaveformDataset's rule (:162-171) for the utterances first_index .. first_index + count - 1 of the data set:
    utterance i gets noise i % n_noise and snr_levels[i % len(snr_levels)] -> (noise ids, SNRs in dB), two lists"""
    snr_levels = list(snr_levels)
    if not snr_levels or n_noise < 1:
        raise ValueError("mix_assignment: at least one SNR level and one noise signal are needed")
    idx = range(first_index, first_index + count)
    return [i % n_noise for i in idx], [float(snr_levels[i % len(snr_levels)]) for i in idx]


def mix_batch(clean, noise_bank_, snr_levels, first_index=0, lengths=None):
    """mix_at_snr with WaveformDataset's assignment: utterance first_index + i of the data set gets
    snr_levels[(first_index + i) % len(snr_levels)] and noise (first_index + i) % len(noise_bank_) -> (noisy, scale)"""
    bank = noise_bank(noise_bank_)
    ids, snr = mix_assignment(clean.shape[0], bank.count, snr_levels, first_index)
    return mix_at_snr(clean, bank, ids, snr, lengths)


class CurriculumBatch(NamedTuple):
    """what curriculum_batch returns: the mix, the channels-last spectra the models consume, the mask target, the mix scales"""
    noisy: torch.Tensor
    noisy_real: torch.Tensor
    noisy_imag: torch.Tensor
    clean_real: torch.Tensor
    clean_imag: torch.Tensor
    mask: Optional[torch.Tensor]
    scale: torch.Tensor


@torch.no_grad()
def curriculum_batch(clean, noise_bank_, snr_levels, mask_type, first_index=0, lengths=None, p=0.5, middle_value=None):
    """One training batch of a curriculum stage, made on the device: the mix of mix_batch, the spectra of the mix and of the
    clean utterances [B, T, F], and the oracle mask [B, T, F] of `mask_type` ('irm', 'pcirm', 'opt_pcirm' or None) - directly the
    `oracle_mask` of MSEMaskLoss for a [B, T, F] prediction.  Nothing carries autograd history.
      'irm'       masks.compute_irm(|C|, |sN|, p)
      'pcirm'     masks.compute_pcirm of |C|, |sN|, the correlation coefficients of (|Y|, |C|, |sN|) and the phase differences
                  arg C - arg Y, arg N - arg Y (a zero bin counts as phase 0)
      'opt_pcirm' that PCIRM through masks.quantize_pcirm(., compute_snr_boundaries()[0], middle_value)
    The STFT is linear: it is taken of `clean` and of the unscaled noise rows (functional.stft, exact fp32), and one
    memory-bound kernel forms Y = C + scale N and the mask from them.  `clean` must be zero from lengths[i] on.
    get_stage(epoch)['snr_levels'] is a value for `snr_levels`; the mask kind is the caller's choice."""
    from ..masks.opt_pcirm import compute_snr_boundaries, quantizer_table
    if mask_type not in ops.MASK_KINDS:
        raise ValueError("curriculum_batch: mask_type must be 'irm', 'pcirm', 'opt_pcirm' or None; got %r" % (mask_type,))
    if mask_type == "irm" and not p > 0:
        raise ValueError("curriculum_batch: p must be positive; got %r" % (p,))
    bank = noise_bank(noise_bank_)
    ids, snr = mix_assignment(clean.shape[0], bank.count, snr_levels, first_index)
    clean, ids, snr, lens = _mix_args("curriculum_batch", clean, bank, ids, snr, lengths)
    scale = ops.mix_scale(clean, bank.buffer, bank.offsets, ids, snr, lens)
    noisy, rows = ops.mix_apply(clean, bank.buffer, bank.offsets, ids, scale, lens, want_rows=True)
    fft, hop, win = config.FFT_SIZE, config.HOP_SIZE, config.FRAME_SIZE
    cr, ci = Fn.stft(clean, fft, hop, win)
    nr, ni = Fn.stft(rows, fft, hop, win)
    table, M = (quantizer_table(compute_snr_boundaries()[0], middle_value, clean.device) if mask_type == "opt_pcirm"
                else (None, 0))
    yr, yi, mask = ops.curriculum_mask(cr, ci, nr, ni, scale, mask_type, p=p, table=table, M=M)
    return CurriculumBatch(noisy, yr, yi, cr, ci, mask, scale)


class _Batches:
    """the (noisy, clean) pairs of one pass over a WaveformSet in slices of `index`; iterating enqueues one launch per pair"""

    def __init__(self, wave_set, index, batch_size, drop_last):
        self.set, self.index, self.batch_size = wave_set, index, int(batch_size)
        n = index.numel()
        self.count = n // self.batch_size if drop_last else -(-n // self.batch_size)

    def __len__(self):
        return self.count

    def __iter__(self):
        for k in range(self.count):
            yield self.set.batch(self.index[k * self.batch_size:(k + 1) * self.batch_size])


class WaveformSet:
    """WaveformDataset (training/conformer_pipeline.py:153-189) on the device.  clean_list: the data set's files in order, each a
    1-D numpy array or tensor (host or device), or None for a file that failed to load; noise_signals: 1-D device tensors as a
    dict or list in the reference's key order, or a NoiseBank.  An entry is kept when it has config.FRAME_SIZE * 4 samples; entry
    i - its position in clean_list, skipped entries counted - is mixed with noise i % n_noise at snr_levels[i % len(snr_levels)].
    Held: the kept clean utterances cut to max_len, back to back (`clean` fp32, `offsets` int32 [N + 1]), `file_index` (host
    list), `noise_ids` int32 [N], `scale` fp32 [N] and the NoiseBank: 4 bytes a sample, the mixes are never stored.  `scale` is
    taken once, here, over each utterance's FULL length (ops.mix_scale_varlen), as the reference mixes before it cuts.
    batch(index) makes the (noisy, clean) pair of an int32 device index list in one launch (ops.wave_batch)."""

    def __init__(self, clean_list, noise_signals, snr_levels, fs=None, max_len=None, device=None):
        self.max_len = int(max_len or (fs or config.SAMPLE_RATE) * 4)
        snr_levels = [float(s) for s in snr_levels]
        if self.max_len < 1 or not snr_levels:
            raise ValueError("WaveformSet: a positive max_len and at least one SNR level are needed")
        if isinstance(noise_signals, dict):
            noise_signals = list(noise_signals.values())
        self.bank = noise_signals if isinstance(noise_signals, NoiseBank) else NoiseBank(noise_signals)
        dev = self.bank.buffer.device if device is None else torch.device(device)
        kept, self.file_index = [], []
        for i, c in enumerate(clean_list):
            if c is None:
                continue
            c = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))
            if c.dim() != 1:
                raise ValueError("WaveformSet: entry %d has shape %s; 1-D signals are needed" % (i, tuple(c.shape)))
            if c.numel() >= config.FRAME_SIZE * 4:
                kept.append(c)
                self.file_index.append(i)
        if not kept:
            raise ValueError("WaveformSet: no utterance of at least %d samples" % (config.FRAME_SIZE * 4))
        full_len = [c.numel() for c in kept]
        if sum(full_len) > 2 ** 31 - 1:
            raise ValueError("WaveformSet: %d samples; the offset table is int32" % sum(full_len))
        if all(not c.is_cuda for c in kept):                                   # one host-to-device copy for the whole list
            full = torch.cat([c.float() for c in kept]).to(dev)
        else:
            full = torch.cat([c.to(dev, torch.float32) for c in kept])
        pos = np.asarray(self.file_index, dtype=np.int64)
        self.noise_ids = torch.from_numpy((pos % self.bank.count).astype(np.int32)).to(dev)
        self.snr_db = torch.tensor([snr_levels[i % len(snr_levels)] for i in self.file_index], dtype=torch.float32, device=dev)
        full_off = np.concatenate([[0], np.cumsum(full_len)])
        self.scale = ops.mix_scale_varlen(full, torch.from_numpy(full_off.astype(np.int32)).to(dev), self.bank.buffer,
                                          self.bank.offsets, self.noise_ids, self.snr_db, max(full_len))
        self.lengths = [min(n, self.max_len) for n in full_len]
        if self.lengths != full_len:
            full = torch.cat([full[a:a + n] for a, n in zip(full_off[:-1].tolist(), self.lengths)])
        self.clean = full.contiguous()
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int32)).to(dev)

    @classmethod
    def from_padded(cls, clean, lengths, noise_signals, snr_levels, fs=None, max_len=None):
        """clean [N, L] fp32 on the device, row i holding lengths[i] samples (a host sequence or a tensor; None: all of L)"""
        if not torch.is_tensor(clean) or not clean.is_cuda:
            raise RuntimeError("WaveformSet.from_padded: the rows live on the MI355X; got a CPU tensor (there is no CPU fallback)")
        if clean.dim() != 2:
            raise ValueError("WaveformSet.from_padded: clean [N, L] is needed; got shape %s" % (tuple(clean.shape),))
        N, L = clean.shape
        host = [L] * N if lengths is None else [int(v) for v in np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).reshape(-1)]
        if len(host) != N or (N and (min(host) < 0 or max(host) > L)):
            raise ValueError("WaveformSet.from_padded: lengths %r for clean %s" % (host, tuple(clean.shape)))
        return cls([clean[i, :host[i]] for i in range(N)], noise_signals, snr_levels, fs, max_len, device=clean.device)

    def __len__(self):
        return len(self.lengths)

    def batch(self, index):
        """index: int32 device tensor [B] (-1: a zero row) -> (noisy [B, max_len], clean [B, max_len])"""
        if not torch.is_tensor(index) or not index.is_cuda:
            raise RuntimeError("WaveformSet.batch: the index lives on the MI355X; got a host value (there is no CPU fallback)")
        out = ops.wave_batch(self.clean, self.offsets, self.bank.buffer, self.bank.offsets, self.noise_ids, self.scale,
                             index.to(torch.int32).reshape(-1).contiguous(), self.max_len)
        return out[0], out[1]

    def __getitem__(self, idx):
        i, n = int(idx), len(self)
        if not -n <= i < n:                                 # (the sequence protocol ends an iteration on this)
            raise IndexError("WaveformSet: utterance %d of %d" % (i, n))
        noisy, clean = self.batch(torch.tensor([i % n], dtype=torch.int32, device=self.clean.device))
        return noisy[0], clean[0]

    def batches(self, batch_size, order=None, drop_last=False, shuffle=False):
        """an iterable of batch() pairs over the set: in `order` (an int32 device permutation), else in a torch.randperm drawn on
        the device when `shuffle`, else in the stored order.  drop_last leaves the last partial batch out."""
        if int(batch_size) < 1:
            raise ValueError("WaveformSet.batches: batch_size %r" % (batch_size,))
        dev = self.clean.device
        if order is not None:
            if not torch.is_tensor(order) or not order.is_cuda:
                raise RuntimeError("WaveformSet.batches: the order lives on the MI355X; got a host value (there is no CPU fallback)")
            index = order.to(torch.int32).reshape(-1).contiguous()
        elif shuffle:
            index = torch.randperm(len(self), device=dev, dtype=torch.int32)
        else:
            index = torch.arange(len(self), device=dev, dtype=torch.int32)
        return _Batches(self, index, batch_size, drop_last)


class WarmupCosineRule:
    """The LambdaLR of ConformerPipeline.train (:432-441) restated on the host: warmup = max(1, min(5, total // 5)) epochs of
    (e + 1) / warmup, then max(0.01, 0.5 (1 + cos(pi (e - warmup) / max(1, total - warmup)))).  There is no torch optimiser to hand
    a scheduler: lr(epoch) is assigned to FlatAdamW.lr before the epoch."""

    def __init__(self, total_epochs, base_lr=5e-4):
        self.total, self.base_lr = int(total_epochs), float(base_lr)
        self.warmup = max(1, min(5, self.total // 5))

    def multiplier(self, epoch):
        if epoch < self.warmup:
            return (epoch + 1) / self.warmup
        progress = (epoch - self.warmup) / max(1, self.total - self.warmup)
        return max(0.01, 0.5 * (1 + math.cos(math.pi * progress)))

    def lr(self, epoch):
        return self.base_lr * self.multiplier(epoch)


def si_snr_loss(estimated, target):
    """training/conformer_pipeline.py:52-71 - negative mean scale-invariant SNR of `estimated` [..., L] against `target`
    (to minimise).  Differentiable w.r.t. `estimated` (HIP backward kernel)."""
    if not estimated.is_cuda:
        raise RuntimeError("si_snr_loss: HIP path needs device tensors (no CPU fallback)")
    from .. import train
    return train.SiSnrFunction.apply(estimated, target)


class MultiResolutionSTFTLoss(nn.Module):
    """training/conformer_pipeline.py:74-108 - spectral convergence + L1 log-magnitude at three STFT resolutions (Hann
    windows, centre reflect padding), averaged over the resolutions.  Same constructor and method names as the reference;
    the STFTs, the reductions and the backward run on the HIP kernels."""

    def __init__(self, fft_sizes=None, hop_sizes=None, win_sizes=None):
        super().__init__()
        self.fft_sizes = fft_sizes or [256, 512, 1024]
        self.hop_sizes = hop_sizes or [64, 128, 256]
        self.win_sizes = win_sizes or [256, 512, 1024]

    def _sizes(self):
        return tuple(zip(self.fft_sizes, self.hop_sizes, self.win_sizes))

    def _stft_mag(self, x, fft_size, hop_size, win_size):
        """|STFT| laid out [B, F, T] like torch.stft (monitoring / tests; forward() does not materialise it)."""
        if not x.is_cuda:
            raise RuntimeError("MultiResolutionSTFTLoss: HIP path needs device tensors (no CPU fallback)")
        r, i = Fn.stft(x.float(), fft_size, hop_size, win_size)
        return torch.sqrt(r * r + i * i).transpose(1, 2)

    def forward(self, predicted, target):
        if not predicted.is_cuda:
            raise RuntimeError("MultiResolutionSTFTLoss: HIP path needs device tensors (no CPU fallback)")
        from .. import train
        return train.MrStftFunction.apply(predicted, target, self._sizes())


class SpeechEnhancer(HipModule):
    """training/conformer_pipeline.py:218-301: LN(2F) -> Linear -> N ConformerBlocks -> LN ->
    magnitude (sigmoid) / phase (tanh * pi/6) heads -> polar mask applied to the noisy STFT."""

    def __init__(self, n_freq=None, d_model=256, num_blocks=4, num_heads=4, d_ff=1024, kernel_size=31, dropout=0.15):
        super().__init__()
        self.n_freq = n_freq or (config.FFT_SIZE // 2 + 1)
        self.num_heads, self.num_blocks = num_heads, num_blocks
        self.input_norm = nn.LayerNorm(2 * self.n_freq)
        self.input_proj = nn.Linear(2 * self.n_freq, d_model)
        self.blocks = nn.ModuleList([ConformerBlock(d_model, num_heads, d_ff, kernel_size, dropout)
                                     for _ in range(num_blocks)])
        self.output_norm = nn.LayerNorm(d_model)
        self.mag_head = nn.Linear(d_model, self.n_freq)
        self.phase_head = nn.Linear(d_model, self.n_freq)

    def _pack(self, sd):
        F2 = 2 * self.n_freq
        heads_w = torch.cat([sd["mag_head.weight"], sd["phase_head.weight"]], dim=0)
        heads_b = torch.cat([sd["mag_head.bias"], sd["phase_head.bias"]], dim=0)
        with ops.stage("front"):
            proj = ops.pack_linear(sd["input_proj.weight"], sd["input_proj.bias"], k_pad_to=ops.round_up(F2, 64))
        with ops.stage("tail"):
            heads = ops.pack_linear(heads_w, heads_b)
        return {"in_w": sd["input_norm.weight"].float().contiguous(), "in_b": sd["input_norm.bias"].float().contiguous(),
                "proj": proj,
                "blocks": [Fn.pack_block(Fn.sub(sd, "blocks.%d" % i), self.num_heads, i) for i in range(self.num_blocks)],
                "on_w": sd["output_norm.weight"].float().contiguous(), "on_b": sd["output_norm.bias"].float().contiguous(),
                "heads": heads}

    def _train_forward(self, noisy_real, noisy_imag):
        """train() mode: same graph built from autograd nodes whose forward AND backward are HIP kernels
        (train.LNLinearFunction, ConformerBlockFunction via ConformerBlock, PolarMaskFunction)."""
        from .. import train
        nr, ni = noisy_real.float().contiguous(), noisy_imag.float().contiguous()
        B, T, F = nr.shape
        M = B * T
        ldc = ops.round_up(2 * F, 8)
        cat = torch.empty(M, ldc, device=nr.device, dtype=torch.float32)
        ops.pack_spec(nr, ni, cat, M, F, ldc, F)
        x = train.LNLinearFunction.apply(cat, self.input_norm.weight, self.input_norm.bias, self.input_proj.weight,
                                         self.input_proj.bias)
        x = x.reshape(B, T, -1)
        for block in self.blocks:
            x = block(x)
        heads_w = torch.cat([self.mag_head.weight, self.phase_head.weight], dim=0)
        heads_b = torch.cat([self.mag_head.bias, self.phase_head.bias], dim=0)
        logits = train.LNLinearFunction.apply(x.reshape(M, -1), self.output_norm.weight, self.output_norm.bias, heads_w,
                                              heads_b)
        return train.PolarMaskFunction.apply(logits, nr, ni, math.pi / 6)

    def forward(self, noisy_real, noisy_imag):
        self._require_device(noisy_real, noisy_imag)
        if self.training or self._wants_autograd(noisy_real, noisy_imag):
            return self._train_forward(noisy_real, noisy_imag)
        pk = self._packed(self._pack)
        nr, ni = noisy_real.float().contiguous(), noisy_imag.float().contiguous()
        B, T, F = nr.shape
        M = B * T
        dev = nr.device
        ldc = ops.round_up(2 * F, 8)
        cat = torch.empty(M, ldc, device=dev, dtype=torch.float32)
        ops.pack_spec(nr, ni, cat, M, F, ldc, F)
        ld16 = pk["proj"].Kpad
        with ops.stage("front"):
            x16 = torch.zeros(M, ld16, device=dev, dtype=ops.compute_dtype())
            ops.layernorm(cat, pk["in_w"], pk["in_b"], out16=x16)            # D = 2F columns, pad stays zero
            x = ops.linear16(x16, pk["proj"], out_dtype=torch.float32)
        for bp in pk["blocks"]:
            x = Fn.block_forward(x, bp, B, T, self.num_heads)
        with ops.stage("tail"):
            h16 = Fn._ln16(x, pk["on_w"], pk["on_b"])
            logits = ops.linear16(h16, pk["heads"], out_dtype=torch.float32)   # [M, 2F] = mag | phase
        er = torch.empty(B, T, F, device=dev, dtype=torch.float32)
        ei = torch.empty(B, T, F, device=dev, dtype=torch.float32)
        mm = torch.empty(B, T, F, device=dev, dtype=torch.float32)
        ops.polar_mask(logits, logits[:, F:], B, T, F, math.pi / 6, logits.stride(0), nr=nr, ni=ni, er=er, ei=ei,
                       mmag=mm, ld_enh=F)
        return er, ei, mm

    def forward_packed(self, noisy_real, noisy_imag, frame_counts):
        """forward() on a packed batch: noisy_real / noisy_imag [sum_T, F] hold the spectra of utterances of different lengths
        back to back, `frame_counts` their frame counts (a sequence, or the functional.PackedSegments of the pass).  Returns
        (enh_real, enh_imag, mask_mag), each [sum_T, F]; every utterance gets what forward() gives it alone.  eval() only."""
        self._require_device(noisy_real, noisy_imag)
        if self.training or self._wants_autograd(noisy_real, noisy_imag):
            raise RuntimeError("SpeechEnhancer.forward_packed is an inference path: call eval() and pass tensors that do not "
                               "require grad (training takes rectangular batches through forward())")
        seg = frame_counts if isinstance(frame_counts, Fn.PackedSegments) else Fn.PackedSegments(frame_counts)
        nr, ni = noisy_real.float().contiguous(), noisy_imag.float().contiguous()
        if nr.dim() != 2 or nr.shape != ni.shape or nr.shape[0] != seg.sum_T or nr.shape[1] != self.n_freq:
            raise RuntimeError("forward_packed: spectra %s / %s, expected [%d, %d] (sum of the frame counts x n_freq)" % (
                tuple(nr.shape), tuple(ni.shape), seg.sum_T, self.n_freq))
        d_model, H = self.input_proj.out_features, self.num_heads
        if d_model % H != 0 or d_model // H > 256:
            raise NotImplementedError("forward_packed: d_model %d with %d heads (head_dim %s): the packed attention kernels take "
                                      "head_dim <= 256" % (d_model, H, d_model / H))
        pk = self._packed(self._pack)
        M, F = nr.shape
        dev = nr.device
        ldc = ops.round_up(2 * F, 8)
        cat = torch.empty(M, ldc, device=dev, dtype=torch.float32)
        ops.pack_spec(nr, ni, cat, M, F, ldc, F)
        ld16 = pk["proj"].Kpad
        with ops.stage("front"):
            x16 = torch.zeros(M, ld16, device=dev, dtype=ops.compute_dtype())
            ops.layernorm(cat, pk["in_w"], pk["in_b"], out16=x16)
            x = ops.linear16(x16, pk["proj"], out_dtype=torch.float32)
        for bp in pk["blocks"]:
            x = Fn.block_forward(x, bp, None, None, H, seg=seg)
        with ops.stage("tail"):
            h16 = Fn._ln16(x, pk["on_w"], pk["on_b"])
            logits = ops.linear16(h16, pk["heads"], out_dtype=torch.float32)   # [M, 2F] = mag | phase
        er = torch.empty(M, F, device=dev, dtype=torch.float32)
        ei = torch.empty(M, F, device=dev, dtype=torch.float32)
        mm = torch.empty(M, F, device=dev, dtype=torch.float32)
        ops.polar_mask(logits, logits[:, F:], 1, M, F, math.pi / 6, logits.stride(0), nr=nr, ni=ni, er=er, ei=ei, mmag=mm, ld_enh=F)
        return er, ei, mm

    def forward_packed_train(self, noisy_real, noisy_imag, frame_counts):
        """The trainable door to packed batches: _train_forward with the blocks on packed rows.  noisy_real / noisy_imag
        [sum_T, F] hold the spectra of utterances of different lengths back to back, `frame_counts` their frame counts (a
        sequence, or the functional.PackedSegments of the pass).  Returns (enh_real, enh_imag, mask_mag), each [sum_T, F], through
        the same chain of autograd nodes as forward() in train(): LNLinearFunction -> blocks -> LNLinearFunction ->
        PolarMaskFunction.  Attention and the depthwise conv stay inside an utterance; BatchNorm's batch statistics run over
        the sum_T real frames.  In eval() the nodes run without dropout and on the running statistics.  head_dim 64 only."""
        from .. import train
        self._require_device(noisy_real, noisy_imag)
        seg = Fn.packed_frames(frame_counts)
        if noisy_real.dim() != 2 or noisy_real.shape != noisy_imag.shape or noisy_real.shape[0] != seg.sum_T or \
                noisy_real.shape[1] != self.n_freq:
            raise RuntimeError("forward_packed_train: spectra %s / %s, expected [%d, %d] (sum of the frame counts x n_freq)" % (
                tuple(noisy_real.shape), tuple(noisy_imag.shape), seg.sum_T, self.n_freq))
        for block in self.blocks:                         # every refusal before the first launch
            train.check_packed_train(self.input_proj.out_features, self.num_heads,
                                     {"conv.depthwise.weight": block.conv.depthwise.weight}, who="forward_packed_train")
        nr, ni = noisy_real.float().contiguous(), noisy_imag.float().contiguous()
        M, F = nr.shape
        ldc = ops.round_up(2 * F, 8)
        cat = torch.empty(M, ldc, device=nr.device, dtype=torch.float32)
        ops.pack_spec(nr, ni, cat, M, F, ldc, F)
        x = train.LNLinearFunction.apply(cat, self.input_norm.weight, self.input_norm.bias, self.input_proj.weight,
                                         self.input_proj.bias)
        for block in self.blocks:
            x = block._train_forward(x, seg=seg)
        heads_w = torch.cat([self.mag_head.weight, self.phase_head.weight], dim=0)
        heads_b = torch.cat([self.mag_head.bias, self.phase_head.bias], dim=0)
        logits = train.LNLinearFunction.apply(x, self.output_norm.weight, self.output_norm.bias, heads_w, heads_b)
        er, ei, mm = train.PolarMaskFunction.apply(logits, nr.unsqueeze(0), ni.unsqueeze(0), math.pi / 6)
        return er.squeeze(0), ei.squeeze(0), mm.squeeze(0)

    # LayerNorm over 2F needs D passed explicitly: ops.layernorm infers D from x32.shape[1]
    # (cat has ldc >= 2F columns), so view the valid columns.


def compute_loss(model, noisy_real, noisy_imag, clean_wav, clean_real, clean_imag, fft_size=None, hop_size=None,
                 frame_size=None):
    """ConformerPipeline._compute_loss (training/conformer_pipeline.py:539-572): model forward -> iSTFT ->
    SI-SNR + 0.5 * L1 magnitude + multi-resolution STFT.  Returns (total, neg_sisnr) like the reference; `total` carries
    the autograd graph (HIP backward kernels) when the model is in train() mode."""
    from .. import train
    fft_size, hop_size = fft_size or config.FFT_SIZE, hop_size or config.HOP_SIZE
    frame_size = frame_size or config.FRAME_SIZE
    enh_real, enh_imag, _ = model(noisy_real, noisy_imag)
    T = min(enh_real.shape[1], clean_real.shape[1])
    total, aux, _ = train.EnhancerLossFunction.apply(enh_real[:, :T], enh_imag[:, :T], clean_wav, clean_real[:, :T],
                                                     clean_imag[:, :T], fft_size, hop_size, frame_size)
    return total, aux[0]


def compute_path_loss(path, noisy_wav, clean_wav):
    """The objective of ConformerPipeline._compute_loss (training/conformer_pipeline.py:539-572) on the north-star
    composition (EnhancementPath in train() mode): SI-SNR + 0.5 * L1 magnitude + multi-resolution STFT of the enhanced
    spectrum against the clean utterance.  Returns (total, neg_sisnr)."""
    from .. import train
    out = path(noisy_wav, want=("mask", "spectrum"))
    with torch.no_grad():
        # split-bf16 operands on the 16-bit matrix cores (4e-6 relative error): the form the objective's own STFTs use
        cr, ci = Fn.stft_split16(clean_wav.float().contiguous())
    total, aux, _ = train.EnhancerLossFunction.apply(out["enh_real"], out["enh_imag"], clean_wav, cr, ci, Fn.N_FFT, Fn.HOP, Fn.WIN)
    return total, aux[0]


class EnhancementPath(HipModule):
    """North-star composition: PerceptionAgent -> (pool to STFT frames) -> CPEA -> STFT ->
    [EpisodicMemory] -> MaskSynthesisAgent -> apply_mask -> iSTFT, fused in the internal
    channels-last layouts (functional.enhance_path).  Glue G1-G3: DESIGN.md."""

    def __init__(self, sample_rate=16000, use_memory=False):
        super().__init__()
        self.perception = PerceptionAgent(sample_rate=sample_rate)
        self.cpea = CorrelationPhaseEstimationAgent()
        self.msa = MaskSynthesisAgent()
        self.memory = EpisodicMemory() if use_memory else None
        self.sample_rate = sample_rate

    def _pack(self, sd):
        packs = {"pa": Fn.pack_perception(Fn.sub(sd, "perception"), self.sample_rate),
                 "cpea": Fn.pack_cpea(Fn.sub(sd, "cpea"), self.cpea.num_layers),
                 "msa": Fn.pack_msa(Fn.sub(sd, "msa"), self.msa.conformer.num_blocks, self.msa.conformer.num_heads)}
        if self.memory is not None:
            m = self.memory
            packs["memory"] = (Fn.pack_memory_params(Fn.sub(sd, "memory")), m.key_dim, m.value_dim, m.num_slots,
                               m.temperature)
        return packs

    def _pack_key(self):
        return tuple([ops.policy_key()] + [(p.data_ptr(), p._version) for p in self.parameters()] +
                     [(b.data_ptr(), b._version) for n, b in self.named_buffers() if "usage" not in n and "num_queries" not in n])

    def freeze_perception(self, flag=True):
        """Train CPEA / memory / MaskSynthesisAgent on a frozen front-end: the PerceptionAgent then runs on the inference
        kernels (its GroupNorm-only stack has no train/eval difference, so the forward is the same either way) and keeps
        none of its activations."""
        self.__dict__["_sfm_pa_frozen"] = bool(flag)
        for p in self.perception.parameters():
            p.requires_grad_(not flag)
        return self

    def _train_forward(self, waveform, want=("mask", "wave")):
        """train() mode: PerceptionAgent, pooling (glue G1), CPEA (BPTT), EpisodicMemory, MaskSynthesisAgent, apply_mask and
        iSTFT as HIP autograd nodes; glue G1-G3 as in eval().  With freeze_perception() the front-end runs without autograd."""
        from .. import train
        wave = waveform.float().contiguous()
        B, L = wave.shape
        T = 1 + L // Fn.HOP
        D = self.perception.encoder_channels if hasattr(self.perception, "encoder_channels") else 256
        with torch.no_grad():
            nr, ni = Fn.stft_split16(wave)                   # as the fused inference path: split-bf16 operands, 4e-6 relative error
        if self.__dict__.get("_sfm_pa_frozen", False):
            with torch.no_grad():
                pa = self.perception._packed(lambda sd: Fn.pack_perception(sd, self.sample_rate))     # frozen: packed once
                (rz, sz, hz), _sigma = Fn.perception_forward(wave, pa, latents=False)
                zp = torch.empty(B, T, 2 * D, device=wave.device, dtype=torch.float32)
                ops.pool_time(rz, None, zp, B, rz.shape[1], T, 2 * D, 2 * D, 2 * D, scale=sz, shift=hz)      # glue G1
        else:
            zp = train.PoolTimeFunction.apply(train.perception_latents_train(self.perception, wave), T)     # glue G1
        if zp.requires_grad:
            zp_all, z_half = train.LatentFanoutFunction.apply(zp, D)             # one fused gradient fan-in for the two consumers
        else:
            zp_all, z_half = zp, zp[..., :D]
        z_real, z_imag = zp_all[..., :D].transpose(1, 2), zp_all[..., D:].transpose(1, 2)
        cpea = self.cpea(z_half)
        bias = None
        out = {}
        if self.memory is not None:
            mem = self.memory(train.MeanTimeFunction.apply(zp[..., :self.memory.key_dim]))                # glue G2
            bias = mem["bias"]                                                                            # glue G3
            out.update(mem_bias=mem["bias"], mem_gate=mem["gate"], mem_top=mem["top_indices"], mem_sim=mem["similarity"])
        mr, mi = self.msa(z_real, z_imag, cpea, nr, ni, mag_logit_bias=bias, latents_cl=zp_all)
        er, ei = train.ComplexMulFunction.apply(nr, ni, mr, mi)
        out.update(mask_real=mr, mask_imag=mi, noisy_real=nr, noisy_imag=ni, enh_real=er, enh_imag=ei)
        if "wave" in want:
            out["enhanced"] = train.IstftFunction.apply(er, ei, L, Fn.N_FFT, Fn.HOP, Fn.WIN)
        return out

    def forward(self, waveform, want=("mask", "wave")):
        self._require_device(waveform)
        if self.training and torch.is_grad_enabled():
            return self._train_forward(waveform, want)
        packs = self._packed(self._pack)
        return Fn.enhance_path(waveform.float(), packs, H=self.msa.conformer.num_heads,
                               use_memory=self.memory is not None, want=want)

    def _refuse_ragged(self, waveform, want):
        """what forward_ragged does not take, said before anything is packed or launched (and so without a device)"""
        if self.training or self._wants_autograd(waveform):
            raise RuntimeError("EnhancementPath.forward_ragged is an inference path: call eval() and pass a waveform that does "
                               "not require grad (training takes rectangular batches through forward())")
        if self.memory is not None:
            raise NotImplementedError("EnhancementPath.forward_ragged: use_memory=True has no ragged form (the memory key is a "
                                      "mean over frames)")
        if "latents" in want:
            raise NotImplementedError("EnhancementPath.forward_ragged does not return full-rate latents")

    def forward_ragged(self, waveform, lengths, want=("mask", "wave")):
        """forward() on utterances of different lengths in ONE pass: waveform [B, Lmax] zero-padded (what follows lengths[b]
        samples in row b is never read), lengths a sequence of B ints >= functional.RAGGED_MIN_SAMPLES.  Returns packed results
        (functional.enhance_path_ragged): mask_real / mask_imag [sum_T, 129], sigma [sum_Tpa], enhanced [sum_L], seg, plan -
        every utterance as forward() gives it alone.  eval() only, no memory, no latents."""
        self._refuse_ragged(waveform, want)
        plan = Fn.ragged_plan(lengths)                             # (a short utterance: ValueError, before the device check)
        self._require_device(waveform)
        packs = self._packed(self._pack)
        return Fn.enhance_path_ragged(waveform.float(), plan, packs, H=self.msa.conformer.num_heads, want=want)

    @torch.no_grad()
    def enhance_batch(self, signals):
        """forward_ragged for a list of 1-D signals (numpy arrays or tensors) of different lengths: one page-locked upload of the
        zero-padded batch, one pass, one download of the packed result; returns a list of numpy arrays of the input lengths.
        Splitting a large set into passes is the caller's."""
        sigs = [np.ascontiguousarray(s.detach().cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1)
                for s in signals]
        if not sigs:
            return []
        self._refuse_ragged(torch.empty(0), ("wave",))
        plan = Fn.ragged_plan([s.size for s in sigs])
        dev = next(self.parameters()).device
        stage = torch.zeros(len(sigs), plan.max_rows[0], dtype=torch.float32, pin_memory=True)
        host = stage.numpy()
        for b, s in enumerate(sigs):
            host[b, :s.size] = s
        out = self.forward_ragged(stage.to(dev, non_blocking=True), plan, want=("wave",))
        y = out["enhanced"].cpu().numpy()
        return np.split(y, plan.seg.sample_offsets[1:-1])


class ConformerPipeline:
    """training/conformer_pipeline.py:308-685 without its file search and audio loading: train (:403) on two WaveformSets, the
    training step (_train_epoch :484, _validate :574, _compute_loss :539), model I/O (:611-649) and enhance_signal (:653).
    model_dir overrides config.MODEL_DIR."""

    def __init__(self, fs=None, device=None, *, model_dir=None):
        self.fs = fs or config.SAMPLE_RATE
        self.model_dir = model_dir or config.MODEL_DIR          # where the checkpoint methods write and look
        self.fft_size, self.hop_size, self.frame_size = config.FFT_SIZE, config.HOP_SIZE, config.FRAME_SIZE
        if not torch.cuda.is_available():
            raise RuntimeError("ConformerPipeline (HIP build) needs an MI355X; there is no CPU fallback")
        self.device = torch.device(device or "cuda")
        self.model = None
        self.use_amp = True           # :334 `use_amp = device.type == 'cuda'`: fp16 operands + dynamic loss scale (make_optimizer)
        self.use_graph = False        # True: enhance_signal replays one hipGraph per signal length (graph.GraphedForward)
        self._graphed = None
        self.history = []             # train(): (train_loss, train_sisnr, val_loss, val_sisnr, lr) per epoch
        self.optimizer = self.scaler = None

    def _compute_loss(self, noisy_real, noisy_imag, clean_wav, clean_real, clean_imag, mr_stft_fn):
        """training/conformer_pipeline.py:539-572: model forward -> iSTFT -> SI-SNR + 0.5 * L1 magnitude +
        multi-resolution STFT; returns (total, neg_sisnr).  With the reference's default resolutions the whole objective is
        one fused autograd node (compute_loss); any other `mr_stft_fn` is composed from the stand-alone nodes."""
        default = isinstance(mr_stft_fn, MultiResolutionSTFTLoss) and mr_stft_fn._sizes() == tuple(Fn.MR_STFT)
        if default:
            return compute_loss(self.model, noisy_real, noisy_imag, clean_wav, clean_real, clean_imag, self.fft_size,
                                self.hop_size, self.frame_size)
        from .. import train
        enh_real, enh_imag, _ = self.model(noisy_real, noisy_imag)
        T = min(enh_real.shape[1], clean_real.shape[1])
        enh_real, enh_imag = enh_real[:, :T], enh_imag[:, :T]
        enh_wav = train.IstftFunction.apply(enh_real, enh_imag, clean_wav.shape[-1], self.fft_size, self.hop_size, self.frame_size)
        loss_sisnr = si_snr_loss(enh_wav, clean_wav)
        loss_mag = train.L1MagnitudeFunction.apply(enh_real, enh_imag, clean_real[:, :T], clean_imag[:, :T])
        loss_stft = mr_stft_fn(enh_wav, clean_wav)
        return loss_sisnr + 0.5 * loss_mag + loss_stft, loss_sisnr

    # -- the training step (training/conformer_pipeline.py:424-429, 442, 484-537) -----------------------------------------
    def make_optimizer(self, params=None, sync=None):
        """(optimizer, scaler) of ConformerPipeline.train: AdamW(lr 5e-4, betas (0.9, 0.98), weight_decay 0.01) with the
        gradient clip 5.0 of :514 folded in (optim.FlatAdamW), and torch.amp.GradScaler('cuda') of :442 when `use_amp`
        (optim.DynamicLossScale: the same scale / growth / backoff rule, kept on the device)."""
        from ..optim import FlatAdamW, DynamicLossScale
        opt = FlatAdamW(list(params if params is not None else self.model.parameters()), lr=5e-4, betas=(0.9, 0.98),
                        weight_decay=0.01, max_norm=5.0, sync=sync)
        return opt, (DynamicLossScale(self.device) if self.use_amp else None)

    def _train_epoch(self, loader, optimizer, mr_stft_fn, scaler):
        """training/conformer_pipeline.py:484-537 with the reference's call order; `optimizer` = optim.FlatAdamW, `scaler` =
        optim.DynamicLossScale or None.  What the reference does on the host per step happens on the device here: the
        `torch.isnan(loss) or torch.isinf(loss): continue` of :509 is the optimiser's skip flag, clip_grad_norm_(5.0) its clip
        coefficient, `loss.item()` a device-side accumulation that is read ONCE at the end of the epoch."""
        self.model.train()
        acc = torch.zeros(3, device=self.device, dtype=torch.float64)           # sum loss, sum SI-SNR, batches counted
        for noisy, clean in loader:
            noisy = noisy.to(self.device, non_blocking=True)
            clean = clean.to(self.device, non_blocking=True)
            optimizer.zero_grad()
            noisy_real, noisy_imag = batch_stft(noisy, self.fft_size, self.hop_size, self.frame_size)
            clean_real, clean_imag = batch_stft(clean, self.fft_size, self.hop_size, self.frame_size)
            loss, neg_sisnr = self._compute_loss(noisy_real, noisy_imag, clean, clean_real, clean_imag, mr_stft_fn)
            if scaler is not None:
                scaler.scale(loss).backward()
                scaler.unscale_(optimizer)
                scaler.step(optimizer, loss=loss)            # NaN / Inf loss -> skipped on the device (:509), clip 5.0 (:514)
                scaler.update()
            else:
                loss.backward()
                optimizer.step(loss=loss)
            with torch.no_grad():
                ok = torch.isfinite(loss.detach()).double()
                acc += torch.stack([torch.nan_to_num(loss.detach().double()) * ok,
                                    -torch.nan_to_num(neg_sisnr.detach().double()) * ok, ok])
        a = acc.cpu()
        n = max(float(a[2]), 1.0)
        return float(a[0]) / n, float(a[1]) / n

    @torch.no_grad()
    def _validate(self, loader, mr_stft_fn):
        """training/conformer_pipeline.py:574-609: the objective in eval() mode, averaged over the batches."""
        self.model.eval()
        acc = torch.zeros(3, device=self.device, dtype=torch.float64)
        for noisy, clean in loader:
            noisy, clean = noisy.to(self.device, non_blocking=True), clean.to(self.device, non_blocking=True)
            noisy_real, noisy_imag = batch_stft(noisy, self.fft_size, self.hop_size, self.frame_size)
            clean_real, clean_imag = batch_stft(clean, self.fft_size, self.hop_size, self.frame_size)
            loss, neg_sisnr = self._compute_loss(noisy_real, noisy_imag, clean, clean_real, clean_imag, mr_stft_fn)
            ok = torch.isfinite(loss).double()                                  # :601 non-finite batches are not counted
            acc += torch.stack([torch.nan_to_num(loss.double()) * ok, -torch.nan_to_num(neg_sisnr.double()) * ok, ok])
        a = acc.cpu()
        n = max(float(a[2]), 1.0)
        return float(a[0]) / n, float(a[1]) / n

    # -- the loop (training/conformer_pipeline.py:403-484) ------------------------------------------------------------------
    def _new_model(self):
        return SpeechEnhancer(n_freq=self.fft_size // 2 + 1, d_model=256, num_blocks=4, num_heads=4, d_ff=1024, kernel_size=31,
                              dropout=0.15)

    def train(self, train_set, test_set, epochs=None, *, seed=None, order=None, batch_size=8, verbose=True):
        """ConformerPipeline.train on two WaveformSets: `epochs or 50` epochs of _train_epoch over shuffled full batches and
        _validate over all of test_set in its order, the rate of WarmupCosineRule assigned before each epoch, best_conformer.pt
        written when the validation loss improves.  self.history: (train_loss, train_sisnr, val_loss, val_sisnr, lr) per epoch,
        lr the rate the epoch ran at.  seed: torch.manual_seed before the model is built (the initial weights, the dropout seeds
        and the shuffles follow it).  order: instead of the shuffles, one int32 device permutation for every epoch or a sequence
        of one per epoch.  An epoch's data never touches the host: each batch is one ops.wave_batch launch."""
        total_epochs = epochs or 50
        if seed is not None:
            torch.manual_seed(seed)
        self.model = self._new_model().to(self.device)
        self._graphed = None
        mr_stft_loss = MultiResolutionSTFTLoss()
        optimizer, scaler = self.optimizer, self.scaler = self.make_optimizer()        # (kept: their stats() after the run)
        rule = WarmupCosineRule(total_epochs, optimizer.lr)
        if verbose:
            print(f"\n  Model: {sum(p.numel() for p in self.model.parameters() if p.requires_grad):,} parameters -> {self.device}")
            print(f"\n{'=' * 60}")
            print(f"  DCSE Training: {total_epochs} epochs")
            print(f"  Loss: SI-SNR + L1 Mag + Multi-Resolution STFT")
            print(f"  Optimizer: AdamW (lr={rule.base_lr:.0e}, wd={optimizer.weight_decay})")
            print(f"  Warmup: {rule.warmup} epochs, then cosine decay")
            print(f"  Gradient clip: {optimizer.max_norm}, AMP: {'ON' if self.use_amp else 'OFF'}")
            print(f"{'=' * 60}")
        best_val_loss = float('inf')
        self.history = []
        for epoch in range(total_epochs):
            lr = optimizer.lr = rule.lr(epoch)
            epoch_order = order if order is None or torch.is_tensor(order) else order[epoch]
            train_loss, train_sisnr = self._train_epoch(
                train_set.batches(batch_size, order=epoch_order, drop_last=True, shuffle=True), optimizer, mr_stft_loss, scaler)
            val_loss, val_sisnr = self._validate(test_set.batches(batch_size), mr_stft_loss)
            improved = val_loss < best_val_loss
            if improved:
                best_val_loss = val_loss
                self._save_best()
            self.history.append((train_loss, train_sisnr, val_loss, val_sisnr, lr))
            if verbose:                                      # (the reference prints the rate its scheduler has just stepped to)
                print(f"  Epoch {epoch + 1:3d}/{total_epochs} | "
                      f"Train: {train_loss:.4f} (SI-SNR: {train_sisnr:+.2f}) | "
                      f"Val: {val_loss:.4f} (SI-SNR: {val_sisnr:+.2f}) | "
                      f"LR: {rule.lr(epoch + 1):.2e} {'*' if improved else ''}")
        if verbose:
            print(f"\n  Best validation loss: {best_val_loss:.4f}")

    # -- model I/O (training/conformer_pipeline.py:611-649): {'model_state', 'model_class'} checkpoints ----------------
    def _checkpoint(self):
        return {"model_state": {k: v.detach().cpu() for k, v in self.model.state_dict().items()}, "model_class": "SpeechEnhancer"}

    def _save_best(self):
        os.makedirs(self.model_dir, exist_ok=True)
        torch.save(self._checkpoint(), os.path.join(self.model_dir, "best_conformer.pt"))

    def save_model(self, filename="conformer_final.pt"):
        if self.model is None:
            return
        os.makedirs(self.model_dir, exist_ok=True)
        path = os.path.join(self.model_dir, filename)
        torch.save(self._checkpoint(), path)
        print(f"  + Model saved: {path}")

    def load_model(self, path=None):
        if path is None:
            path = os.path.join(self.model_dir, "conformer_final.pt")
            if not os.path.exists(path):
                path = os.path.join(self.model_dir, "best_conformer.pt")
        # tensors only: a checkpoint is {'model_state': state_dict, 'model_class': str} (the reference unpickles with
        # weights_only=False; nothing in its checkpoints needs that)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.model = SpeechEnhancer(n_freq=self.fft_size // 2 + 1, d_model=256, num_blocks=4, num_heads=4, d_ff=1024,
                                    kernel_size=31, dropout=0.15)
        self.model.load_state_dict(ckpt["model_state"])
        self.model.to(self.device).eval()
        self._graphed = None          # a captured hipGraph replays the OLD model's packed weights
        print(f"  + Conformer loaded: {path}")

    @torch.no_grad()
    def enhance_signal(self, noisy_signal):
        if self.model is None:
            raise RuntimeError("No model loaded.")
        self.model.eval()
        x = torch.from_numpy(np.asarray(noisy_signal, dtype=np.float32)).unsqueeze(0).to(self.device)
        if self.use_graph:
            if self._graphed is None:
                from ..graph import GraphedForward
                self._graphed = GraphedForward(self._enhance_device)
            y = self._graphed(x)
        else:
            y = self._enhance_device(x)
        return y.squeeze(0).cpu().numpy()

    @torch.no_grad()
    def enhance_batch(self, noisy_signals, max_frames=None):
        """enhance_signal for a list of signals of different lengths (1-D numpy arrays or tensors) in packed passes: no padding,
        every result equal to what enhance_signal gives that signal alone; returns a list of numpy arrays of the same lengths.
        Per pass: one host-to-device copy of the concatenated samples, one forward over all frames, one copy back.
        max_frames: upper bound on the frames of a pass (functional.packed_segments); default: one pass."""
        if self.model is None:
            raise RuntimeError("No model loaded.")
        sigs = [np.ascontiguousarray(s.detach().cpu().numpy() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1)
                for s in noisy_signals]
        if not sigs:
            return []
        self.model.eval()
        out = []
        for seg in Fn.packed_segments([s.size for s in sigs], self.fft_size, self.hop_size, max_frames):
            # the samples are concatenated straight into a page-locked staging buffer: one asynchronous copy to the device
            stage = torch.empty(seg.sum_L, dtype=torch.float32, pin_memory=True)
            np.concatenate(sigs[seg.start:seg.stop], out=stage.numpy())
            x = stage.to(self.device, non_blocking=True)
            y = self._enhance_packed_device(x, seg).cpu().numpy()
            out.extend(np.split(y, seg.sample_offsets[1:-1]))             # views of the pass's result, no second copy
        return out

    def _enhance_packed_device(self, x, seg):
        """the device part of a packed pass: samples [sum_L] of the pass's signals back to back -> enhanced samples [sum_L]"""
        nr, ni = Fn.stft_packed(x, seg, self.fft_size, self.hop_size, self.frame_size)
        er, ei, _ = self.model.forward_packed(nr, ni, seg)
        return Fn.istft_packed(er, ei, seg, self.fft_size, self.hop_size, self.frame_size)

    @torch.no_grad()
    def evaluate_batch(self, clean_signals, noisy_signals, fs=None, max_frames=None, metrics=("stoi", "pesq", "ssnr"),
                       return_enhanced=False):
        """The inner loop of the reference's evaluate (main.py:315-359) for one list of test files: enhance every noisy signal
        and score the noisy and the enhanced signal against the clean one (compute_stoi, compute_pesq, compute_ssnr on
        clean[:ml], x[:ml]), in packed passes.  Two lists of 1-D signals of any lengths; every pair is cut to its shorter member.
        Returns {"noisy": {metric: float64 numpy [N]}, "enhanced": {...}} in the caller's order, and with return_enhanced
        "signals": the list enhance_batch returns.  Per pass: one host-to-device copy (noisy and clean samples), STFT, forward
        and iSTFT as enhance_batch, evaluation.compute_metrics_packed twice, ONE copy back of the [2, metrics, B] scores; the
        enhanced samples leave the device only with return_enhanced.  max_frames: as enhance_batch."""
        from ..evaluation import packed as pk
        if self.model is None:
            raise RuntimeError("No model loaded.")
        metrics = pk._check_metrics(metrics)
        clean, noisy, passes = pk.plan_evaluation(clean_signals, noisy_signals, self.fft_size, self.hop_size, max_frames)
        N = len(noisy)
        res = {k: {m: np.zeros(N, dtype=np.float64) for m in metrics} for k in ("noisy", "enhanced")}
        if return_enhanced:
            res["signals"] = []
        self.model.eval()
        fs = fs or self.fs
        for seg in passes:
            stage = torch.empty(2, seg.sum_L, dtype=torch.float32, pin_memory=True)
            np.concatenate(noisy[seg.start:seg.stop], out=stage.numpy()[0])
            np.concatenate(clean[seg.start:seg.stop], out=stage.numpy()[1])
            both = stage.to(self.device, non_blocking=True)
            x, c = both[0], both[1]
            y = self._enhance_packed_device(x, seg)
            shared = {}                                                    # the clean spectra serve both comparisons
            sn = pk.compute_metrics_packed(c, x, seg, fs, metrics, clean_spectra=shared)
            se = pk.compute_metrics_packed(c, y, seg, fs, metrics, clean_spectra=shared)
            scores = torch.stack([torch.stack([d[m] for m in metrics]) for d in (sn, se)]).cpu().numpy()
            for k, side in enumerate(("noisy", "enhanced")):
                for j, m in enumerate(metrics):
                    res[side][m][seg.start:seg.stop] = scores[k, j]
            if return_enhanced:
                res["signals"].extend(np.split(y.cpu().numpy(), seg.sample_offsets[1:-1]))
        return res

    def _enhance_device(self, x):
        nr, ni = batch_stft(x, self.fft_size, self.hop_size, self.frame_size)
        er, ei, _ = self.model(nr, ni)
        return batch_istft(er, ei, self.fft_size, self.hop_size, self.frame_size, length=x.shape[-1])
