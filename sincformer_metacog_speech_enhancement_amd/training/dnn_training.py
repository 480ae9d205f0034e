"""Mirror of the training half of training/pipeline.py: SpeechEnhancementDataset (:217-289) as FrameSet, a frame set kept on the
device at the D raw columns, and TrainingPipeline (:296-335, 518-817) with train, _train_epoch, _validate, _rbm_pretrain, _save_best,
save_model, load_model and enhance_signal under the reference's names.  A training step never forms the [M, D (2 ctx + 1)] rows:
the first layer gathers, normalises and clips them from the packed frames by index (ops.dnn_layer_indexed), the loss kernel reads the
target rows by the same index and writes the output layer's cotangent under the loss scale (ops.mse_gather_loss), optim.FlatAdam is
the reference's Adam(weight_decay=1e-5) behind clip_grad_norm_(5.0), and the epoch's losses are summed on the device and read once.

Not mirrored: prepare_data, the file search, the .npz cache and the worker pool (:337-516); FrameSet.from_waveforms is the device
form of what they feed."""
import os

import numpy as np
import torch
from torch import nn

from .. import config, ops, optim
from . import pipeline as _pl


def _as_stat(s, K, device):
    s = torch.as_tensor(np.asarray(s, dtype=np.float32) if not torch.is_tensor(s) else s).to(device, torch.float32).reshape(-1)
    if s.numel() != K:
        raise ValueError("FrameSet: statistics of %d values for rows of %d" % (s.numel(), K))
    return s.contiguous()


class FrameSet:
    """SpeechEnhancementDataset on the device, at D columns.  raw_list / mask_list: per-utterance fp32 device tensors raw [T_u, D]
    (FeatureExtractor.extract_frame_features) and mask [T_u', C]; each utterance is cut to min(T_u, T_u') frames and dropped when
    that is 0.  Held: raw [N, D] and mask [N, C] packed, bounds int32 [N, 2] (for every frame the first and the one-past-last packed
    row of its utterance), feat_mean / feat_std (numpy float32 [D (2 context + 1)], what a checkpoint stores) and their device copies
    mean_dev / std_dev.  Statistics that are not given are computed over the context rows of all frames (ops.context_moments: nan /
    inf -> 0, mean and population std in fp64, std < 1e-6 -> 1); given ones are used as they are.  The mask is stored as computed:
    its nan_to_num and clip to [0, 1] happen where a target is read (ops.mse_gather_loss, rows)."""

    def __init__(self, raw_list, mask_list, feat_mean=None, feat_std=None, context=None):
        self.context = config.CONTEXT_FRAMES if context is None else int(context)
        if (feat_mean is None) != (feat_std is None):
            raise ValueError("FrameSet: feat_mean and feat_std go together")
        if len(raw_list) != len(mask_list):
            raise ValueError("FrameSet: %d feature tensors, %d masks" % (len(raw_list), len(mask_list)))
        raws, masks, spans = [], [], []
        for f, m in zip(raw_list, mask_list):
            for name, t in (("raw", f), ("mask", m)):
                if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
                    raise ValueError("FrameSet: %s must be fp32 tensors [T, .]" % name)
                if not t.is_cuda:
                    raise RuntimeError("FrameSet: the frames live on the MI355X; got a CPU tensor (there is no CPU fallback)")
            n = min(f.shape[0], m.shape[0])
            if n > 0:
                raws.append(f[:n].detach())
                masks.append(m[:n].detach())
                spans.append(n)
        if not raws:
            raise ValueError("FrameSet: no frames")
        if len({t.shape[1] for t in raws}) != 1 or len({t.shape[1] for t in masks}) != 1:
            raise ValueError("FrameSet: the utterances differ in their column counts")
        self.raw = torch.cat(raws, dim=0).contiguous()
        self.mask = torch.cat(masks, dim=0).contiguous()
        N, D = self.raw.shape
        if D < 8 or D % 2 or N >= 2 ** 31:
            raise ValueError("FrameSet: %d frames of %d columns; an even D >= 8 and fewer than 2^31 frames are needed" % (N, D))
        ends = np.cumsum(np.asarray(spans, dtype=np.int64))
        starts = ends - np.asarray(spans, dtype=np.int64)
        bounds = np.stack([np.repeat(starts, spans), np.repeat(ends, spans)], axis=1).astype(np.int32)
        self.bounds = torch.from_numpy(bounds).to(self.raw.device)
        self.lengths = list(spans)
        K = D * (2 * self.context + 1)
        if feat_mean is None:
            self.mean_dev, self.std_dev = ops.context_moments(self.raw, self.bounds, self.context)
        else:
            self.mean_dev, self.std_dev = _as_stat(feat_mean, K, self.raw.device), _as_stat(feat_std, K, self.raw.device)
        # what a checkpoint stores: numpy float32 on the host.  A given numpy float32 array is kept as the object it is (:257-259);
        # anything else (a list, a tensor on any device, another dtype) is copied to the host once, here
        self.feat_mean = self._host_stat(feat_mean, self.mean_dev)
        self.feat_std = self._host_stat(feat_std, self.std_dev)

    @staticmethod
    def _host_stat(given, on_device):
        if isinstance(given, np.ndarray) and given.dtype == np.float32 and given.ndim == 1:
            return given
        return on_device.cpu().numpy()

    @classmethod
    def from_padded(cls, raw, mask, lengths=None, feat_mean=None, feat_std=None, context=None):
        """raw [B, T, D], mask [B, T', C] zero-padded batches, lengths: frame counts T_b (None: all of T)"""
        B = raw.shape[0]
        host = [raw.shape[1]] * B if lengths is None else [int(v) for v in np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).reshape(-1)]
        if len(host) != B or mask.shape[0] != B or min(host) < 0 or max(host) > raw.shape[1]:
            raise ValueError("FrameSet.from_padded: frame counts %r for raw %s, mask %s" % (host, tuple(raw.shape), tuple(mask.shape)))
        return cls([raw[b, :host[b]] for b in range(B)], [mask[b, :min(host[b], mask.shape[1])] for b in range(B)], feat_mean, feat_std, context)

    @classmethod
    def from_waveforms(cls, clean, noise, noisy, mask_type, fe=None, lengths=None, feat_mean=None, feat_std=None):
        """the two halves of dnn_frame_pairs without its add_context: fe.extract_frame_features(noisy) and gammatone_mask_target of
        fp32 device waveforms [B, L] (lengths: the sample counts of a zero-padded batch)"""
        fe = _pl._fe_for(fe)
        one_d = noisy.dim() == 1
        mask = _pl.gammatone_mask_target(clean, noise, noisy, mask_type, gfb=fe.gfb, lengths=lengths)
        raw = fe.extract_frame_features(noisy, lengths=lengths)
        if one_d:
            raw, mask = raw.unsqueeze(0), mask.unsqueeze(0)
        return cls.from_padded(raw, mask, _pl._frame_counts(lengths), feat_mean, feat_std, fe.context)

    def __len__(self):
        return self.raw.shape[0]

    @property
    def feature_dim(self):
        return self.raw.shape[1] * (2 * self.context + 1)

    @property
    def mask_dim(self):
        return self.mask.shape[1]

    def bytes_per_frame(self):
        """device bytes held per frame: the raw row, the mask row and the bounds"""
        return 4 * self.raw.shape[1] + 4 * self.mask.shape[1] + 8

    def rows(self, index):
        """-> (features fp32 [M, D (2 context + 1)], masks fp32 [M, C]) of the frames index (int tensor or list): the Dataset's
        normalised, clipped rows and clipped masks, formed with torch arithmetic in fp64.  For inspection, tests and the RBM's
        one-off sample; the training step never calls it."""
        idx = torch.as_tensor(index, device=self.raw.device).reshape(-1).long()
        if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError("FrameSet.rows: indices outside 0 .. %d" % (len(self) - 1))
        b = self.bounds[idx].long()
        off = torch.arange(-self.context, self.context + 1, device=idx.device)
        src = torch.minimum(torch.maximum(idx[:, None] + off[None, :], b[:, :1]), b[:, 1:] - 1)
        f = torch.nan_to_num(self.raw[src].double(), nan=0.0, posinf=0.0, neginf=0.0).reshape(idx.numel(), -1)
        f = ((f - self.mean_dev.double()) / self.std_dev.double()).clamp(-10.0, 10.0).float()
        m = torch.nan_to_num(self.mask[idx], nan=0.0, posinf=1.0, neginf=0.0).clamp(0.0, 1.0)
        return f, m

    def __getitem__(self, idx):
        i, n = int(idx), len(self)
        if not -n <= i < n:                                 # (the sequence protocol ends an iteration on this)
            raise IndexError("FrameSet: frame %d of %d" % (i, n))
        f, m = self.rows([i % n])
        return f[0], m[0]


class PlateauRule:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience, min_lr) with its default relative threshold 1e-4,
    cooldown 0 and eps 1e-8, restated on the host: there is no torch optimiser to hand it, the rate is an argument of FlatAdam.step"""

    def __init__(self, lr, factor=0.5, patience=5, min_lr=1e-6, threshold=1e-4, eps=1e-8):
        self.lr, self.factor, self.patience, self.min_lr, self.threshold, self.eps = float(lr), factor, patience, min_lr, threshold, eps
        self.best, self.num_bad_epochs = float("inf"), 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = metric, 0
        else:
            self.num_bad_epochs += 1
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.num_bad_epochs = 0
        return self.lr


class TrainingPipeline:
    """TrainingPipeline of training/pipeline.py on two FrameSets.  train() follows :518-632: the model from config, Kaiming
    initialisation, optional RBM pre-training, Adam(lr, weight_decay 1e-5) behind the clip to 5.0 under a dynamic loss scale (the
    reference's autocast + GradScaler), ReduceLROnPlateau(0.5, 5, 1e-6), the best validation loss is checkpointed.  Three NaN epochs
    in a row re-initialise the weights and Adam's moments and step count and go on at a tenth of the initial rate; the plateau
    rule's best loss and bad-epoch count and the loss scale are kept.  Checkpoints carry the reference's keys, with feat_mean / feat_std as numpy float32: they
    load there and the reference's load here.  model_dir overrides config.MODEL_DIR.
    Not mirrored: prepare_data, the file search, the .npz cache and the worker pool; FrameSet.from_waveforms is the device form of
    what they feed."""

    def __init__(self, mask_type='pcirm', use_rbm_pretrain=True, model_dir=None, rbm_seed=None):
        self.mask_type = mask_type
        self.use_rbm_pretrain = use_rbm_pretrain
        self.fs = config.SAMPLE_RATE
        self.model = None
        self.feat_mean = None
        self.feat_std = None
        self.feature_dim = None
        self.mask_dim = None
        if not torch.cuda.is_available():
            raise RuntimeError("TrainingPipeline: the training step only runs on an MI355X (there is no CPU fallback)")
        self.device = torch.device('cuda')
        self.model_dir = model_dir or config.MODEL_DIR
        self.rbm_seed = rbm_seed
        self.batch_size = config.DNN_BATCH_SIZE
        self.scaler = None
        self.history = []                                   # (train loss, validation loss, rate) per finished epoch
        self.batch_losses = []                              # the last epoch's per-batch losses, device tensors
        self._rec = None

    # ---- model ---------------------------------------------------------------------------------------------------------------
    def _new_model(self):
        from ..models.dnn import SpeechEnhancementDNN
        return SpeechEnhancementDNN(input_dim=self.feature_dim, hidden_dim=config.DNN_HIDDEN_UNITS, output_dim=self.mask_dim,
                                    num_hidden_layers=config.DNN_HIDDEN_LAYERS, dropout=config.DNN_DROPOUT)

    @staticmethod
    def _init_weights(model):
        for module in model.modules():
            if isinstance(module, nn.Linear):
                with torch.no_grad():
                    nn.init.kaiming_normal_(module.weight, nonlinearity='relu')
                    if module.bias is not None:
                        nn.init.zeros_(module.bias)

    def _optimizer(self, lr):
        return optim.FlatAdam(self.model.parameters(), lr=lr, weight_decay=1e-5, max_norm=5.0)

    # ---- the loop ------------------------------------------------------------------------------------------------------------
    def train(self, train_set, test_set, epochs=None, *, seed=None, order=None, verbose=True):
        epochs = epochs or config.DNN_EPOCHS
        self.feature_dim, self.mask_dim = train_set.feature_dim, train_set.mask_dim
        self.feat_mean, self.feat_std = train_set.feat_mean, train_set.feat_std
        if seed is not None:
            torch.manual_seed(seed)
        self.model = self._new_model()
        self._init_weights(self.model)
        self.model = self.model.to(self.device)
        if self.use_rbm_pretrain:
            self._rbm_pretrain(train_set, verbose=verbose)
        if verbose:
            print(f"\n  Model: {self.model.count_parameters():,} parameters → {self.device}")
        if any(bool(torch.isnan(p).any()) for p in self.model.parameters()):
            self._init_weights(self.model)
        optimizer = self._optimizer(config.DNN_LEARNING_RATE)
        scheduler = PlateauRule(config.DNN_LEARNING_RATE, factor=0.5, patience=5, min_lr=1e-6)
        self.scaler = optim.DynamicLossScale(self.device)
        if verbose:
            print(f"\n{'=' * 60}")
            print(f"  Training: {epochs} epochs, batch={self.batch_size}, AMP=ON, Optimizer=Adam")
            print(f"{'=' * 60}")
        best_val_loss = float('inf')
        nan_count = 0
        self.history = []
        for epoch in range(1, epochs + 1):
            optimizer.lr = scheduler.lr
            train_loss = self._train_epoch(train_set, optimizer, self.scaler, order=order)
            if np.isnan(train_loss) or np.isinf(train_loss):
                nan_count += 1
                if verbose:
                    print(f"  ⚠ Epoch {epoch}: NaN detected! (count={nan_count}/3)")
                if nan_count >= 3:
                    if verbose:
                        print("  ✗ Training diverged. Re-initializing model...")
                    # the reference builds a fresh Adam at a tenth of the rate here.  Reset: the weights (Kaiming again), Adam's
                    # m, v and step count, the rate.  Kept: the plateau rule's best loss and bad-epoch count (the reference's
                    # scheduler lives on too, bound to the optimiser it no longer uses) and the loss scale's state.
                    # (An epoch's loss averages its finite batches, so only an epoch that the record cannot count gets here.)
                    self._init_weights(self.model)
                    optimizer._bump_versions()
                    optimizer.m.zero_()
                    optimizer.v.zero_()
                    optimizer.ctl.zero_()
                    scheduler.lr = config.DNN_LEARNING_RATE * 0.1
                    nan_count = 0
                continue
            nan_count = 0
            val_loss = self._validate(test_set)
            improved = val_loss < best_val_loss
            if improved:
                best_val_loss = val_loss
                self._save_best()
            scheduler.step(val_loss)
            self.history.append((train_loss, val_loss, scheduler.lr))
            if verbose:
                print(f"  Epoch {epoch:3d}/{epochs} │ Train: {train_loss:.6f} │ Val: {val_loss:.6f} │ LR: {scheduler.lr:.2e} "
                      f"{'★' if improved else ''}")
        if verbose:
            print(f"\n  Best validation loss: {best_val_loss:.6f}")

    def _record(self):
        if self._rec is None:
            self._rec = torch.zeros(4, device=self.device, dtype=torch.float64)
        self._rec.zero_()
        return self._rec

    def _order(self, n, order):
        if order is None:
            return torch.randperm(n, device=self.device, dtype=torch.int32)
        order = torch.as_tensor(order).to(self.device, torch.int32).reshape(-1).contiguous()
        return order

    def _train_epoch(self, train_set, optimizer, scaler, order=None):
        """one epoch over a device permutation (or `order`) in slices of the batch size, the last one ragged; nothing synchronises
        until the epoch's record is read: -> sum of the finite batch losses / max(their number, 1)"""
        self.model.train()
        rec = self._record()
        self.batch_losses = []
        perm = self._order(len(train_set), order)
        ls = scaler._alloc(self.device) if scaler is not None and scaler.enabled else None
        from ..train import DnnIndexedFunction
        for s in range(0, perm.numel(), self.batch_size):
            index = perm[s:s + self.batch_size]
            optimizer.zero_grad()
            y = self.model.forward_indexed(train_set, index)
            loss, dz = ops.mse_gather_loss(y.detach(), train_set.mask, index, loss_scale=ls, rec=rec, ctl=optimizer.ctl)
            self.batch_losses.append(loss)                  # device tensors: nothing is read here
            grads = DnnIndexedFunction.step_gradients(y, dz)
            torch.cat([g.reshape(-1) for g in grads], out=optimizer.sync.flat)
            optimizer.step(scaler=scaler)
        return self._epoch_loss(rec)

    @torch.no_grad()
    def _validate(self, test_set):
        self.model.eval()
        rec = self._record()
        index_all = torch.arange(len(test_set), device=self.device, dtype=torch.int32)
        for s in range(0, len(test_set), self.batch_size):
            index = index_all[s:s + self.batch_size]
            y = self.model.forward_indexed(test_set, index)
            ops.mse_gather_loss(y, test_set.mask, index, need_dz=False, rec=rec)
        return self._epoch_loss(rec)

    @staticmethod
    def _epoch_loss(rec):
        total, count = rec[:2].tolist()                     # the epoch's one readback
        return total / max(count, 1.0)

    def _rbm_pretrain(self, train_set, verbose=True):
        """the first min(50000, N) rows of one epoch's order, materialised once, go to rbm_pretrain (:712-759)"""
        if verbose:
            print(f"\n{'=' * 60}\n  RBM Pre-training (on normalized features)\n{'=' * 60}")
        order = torch.randperm(len(train_set), device=self.device)[:50000]
        features, _ = train_set.rows(order)
        return _pl.rbm_pretrain(self.model, features, max_samples=50000, seed=self.rbm_seed, verbose=verbose)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------
    def _checkpoint(self):
        return {'model_state': {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                'mask_type': self.mask_type, 'feature_dim': self.feature_dim, 'mask_dim': self.mask_dim,
                'feat_mean': None if self.feat_mean is None else np.asarray(self.feat_mean, dtype=np.float32),
                'feat_std': None if self.feat_std is None else np.asarray(self.feat_std, dtype=np.float32)}

    def _save_best(self):
        os.makedirs(self.model_dir, exist_ok=True)
        path = os.path.join(self.model_dir, f'best_{self.mask_type}.pt')
        torch.save(self._checkpoint(), path)
        return path

    def save_model(self, filename=None):
        if self.model is None:
            print("  ✗ No model to save.")
            return None
        os.makedirs(self.model_dir, exist_ok=True)
        path = os.path.join(self.model_dir, filename or f'dnn_{self.mask_type}_final.pt')
        torch.save(dict(self._checkpoint(), device=str(self.device)), path)
        return path

    def load_model(self, path=None):
        if path is None:
            path = os.path.join(self.model_dir, f'best_{self.mask_type}.pt')
        checkpoint = torch.load(path, map_location='cpu', weights_only=False)
        self.feature_dim = checkpoint['feature_dim']
        self.mask_dim = checkpoint['mask_dim']
        self.feat_mean = checkpoint.get('feat_mean')
        self.feat_std = checkpoint.get('feat_std')
        self.model = self._new_model()
        self.model.load_state_dict(checkpoint['model_state'])
        self.model = self.model.to(self.device).eval()
        return self.model

    @torch.no_grad()
    def enhance_signal(self, noisy, lengths=None):
        """dnn_enhance_signal with the pipeline's model and statistics: fp32 device waveforms [B, L] or [L] -> the same shape"""
        if self.model is None:
            raise RuntimeError("TrainingPipeline.enhance_signal: train() or load_model() first")
        self.model.eval()
        return _pl.dnn_enhance_signal(self.model, noisy, lengths=lengths, feat_mean=self.feat_mean, feat_std=self.feat_std)
