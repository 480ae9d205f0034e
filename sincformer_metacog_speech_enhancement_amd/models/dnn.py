"""Host-side mirror of models/dnn.py (SpeechEnhancementDNN :22-113, create_dnn :116-132): the paper's mask estimator,
[Linear, ReLU, Dropout] x num_hidden_layers, Linear, Sigmoid, on csrc/dnn.hip.  The torch submodules hold the parameters (same
state_dict keys, shapes and default init as the reference: a checkpoint's model_state loads as it is) and are never called."""
import numpy as np
import torch
from torch import nn

from .. import config, ops
from .._hostmod import HipModule


class SpeechEnhancementDNN(HipModule):
    def __init__(self, input_dim=None, hidden_dim=None, output_dim=None, num_hidden_layers=None, dropout=None):
        super().__init__()
        # (`x or default`, as the reference writes it: 0 selects the default too, so dropout=0 gives 0.2)
        self.input_dim = input_dim or 594
        self.hidden_dim = hidden_dim or config.DNN_HIDDEN_UNITS
        self.output_dim = output_dim or config.NUM_CHANNELS
        self.num_hidden_layers = num_hidden_layers or config.DNN_HIDDEN_LAYERS
        self.dropout_rate = dropout or config.DNN_DROPOUT
        layers = [nn.Linear(self.input_dim, self.hidden_dim), nn.ReLU(), nn.Dropout(self.dropout_rate)]
        for _ in range(self.num_hidden_layers - 1):
            layers += [nn.Linear(self.hidden_dim, self.hidden_dim), nn.ReLU(), nn.Dropout(self.dropout_rate)]
        layers += [nn.Linear(self.hidden_dim, self.output_dim), nn.Sigmoid()]
        self.network = nn.Sequential(*layers)

    def _linears(self):
        return [m for m in self.network if isinstance(m, nn.Linear)]

    def _packs(self):
        def build(sd):
            packs = []
            for i in range(self.num_hidden_layers + 1):
                w, b = sd["network.%d.weight" % (3 * i)], sd["network.%d.bias" % (3 * i)]
                packs.append(ops.pack_linear(w, b, k_pad_to=ops.round_up(w.shape[1], 8)))
            return packs
        return self._packed(build)

    def _tail(self, h, packs):
        """the layers behind the first: rows16 launches, the last with the sigmoid and an fp32 result"""
        for pw in packs[1:-1]:
            h = ops.dnn_layer(h, pw, act="relu")
        return ops.dnn_layer(h, packs[-1], act="sigmoid", out_dtype=torch.float32)

    def forward(self, x):
        """x fp32 device rows [..., input_dim] -> fp32 [..., output_dim].  eval() without autograd: one sfm_dnn_layer launch per
        Linear, the input converted while the first one stages it; train(), or autograd wanted: train.DnnFunction."""
        self._require_device(x)
        if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] != self.input_dim or x.numel() == 0:
            raise ValueError("SpeechEnhancementDNN: fp32 rows [..., %d] are needed; got %s %s" % (self.input_dim, x.dtype, tuple(x.shape)))
        rows = x.reshape(-1, self.input_dim)
        if self.training or self._wants_autograd(x):
            from .. import train
            p = float(self.dropout_rate) if self.training else 0.0
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p > 0 else 0
            params = [t for m in self._linears() for t in (m.weight, m.bias)]
            y = train.DnnFunction.apply(rows, p, seed, *params)
        else:
            rows = rows.detach()
            if rows.stride(-1) != 1:
                rows = rows.contiguous()
            packs = self._packs()
            y = self._tail(ops.dnn_layer(rows, packs[0], act="relu"), packs)
        return y.reshape(*x.shape[:-1], self.output_dim)

    def forward_frames(self, raw, feat_mean=None, feat_std=None, lengths=None):
        """raw [B, T, D] or [T, D] fp32 (FeatureExtractor.extract_frame_features), input_dim = D (2 CONTEXT_FRAMES + 1) ->
        [B, T, output_dim]: forward(FeatureExtractor.add_context(raw, feat_mean, feat_std, lengths)), padding rows included, with
        the context rows gathered, normalised and clipped inside the first layer's launch: the [B, T, input_dim] tensor is never
        written.  lengths: frame counts T_b of a zero-padded batch.  When autograd is wanted the rows are materialised (the first
        layer's weight gradient needs them)."""
        self._require_device(raw)
        ctx = config.CONTEXT_FRAMES
        if raw.dtype != torch.float32 or raw.dim() not in (2, 3) or raw.numel() == 0 or raw.shape[-1] * (2 * ctx + 1) != self.input_dim:
            raise ValueError("SpeechEnhancementDNN.forward_frames: fp32 [T, D] or [B, T, D] with D * %d = %d is needed; got %s %s"
                             % (2 * ctx + 1, self.input_dim, raw.dtype, tuple(raw.shape)))
        if (feat_mean is None) != (feat_std is None):
            raise ValueError("SpeechEnhancementDNN.forward_frames: feat_mean and feat_std go together")
        two_d = raw.dim() == 2
        f = raw.detach().reshape(1, *raw.shape) if two_d else raw.detach()
        f = f.contiguous()
        B, T, _ = f.shape
        stats = []
        for s in (feat_mean, feat_std):
            if s is not None:
                s = torch.as_tensor(np.asarray(s, dtype=np.float32) if not torch.is_tensor(s) else s).to(f.device, torch.float32).reshape(-1)
                if s.numel() != self.input_dim:
                    raise ValueError("SpeechEnhancementDNN.forward_frames: statistics of %d values for rows of %d" % (s.numel(), self.input_dim))
                stats.append(s.contiguous())
        frames = None
        if lengths is not None:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
            if host.size != B or int(host.min()) < 0 or int(host.max()) > T:
                raise ValueError("SpeechEnhancementDNN.forward_frames: frame counts %r for %d utterances of %d frames" % (host.tolist(), B, T))
            frames = torch.from_numpy(host.astype(np.int32)).to(f.device)
        mean, std = stats if stats else (None, None)
        if self.training or self._wants_autograd(raw):
            y = self.forward(ops.feature_context(f, ctx, L=T, frame=1, hop=1, mean=mean, std=std, clip=10.0, lengths=frames))
            return y[0] if two_d else y
        packs = self._packs()
        h = ops.dnn_layer(f, packs[0], act="relu", context=ctx, frames=frames, mean=mean, std=std)
        y = self._tail(h, packs).reshape(B, T, self.output_dim)
        return y[0] if two_d else y

    def forward_indexed(self, frames, index):
        """frames: a training.FrameSet (raw [N, D], bounds, feat_mean / feat_std on the device), index int32 device tensor [M] of
        packed frames (repeats allowed, < 0: a zero input row) -> fp32 [M, output_dim]: forward(frames.rows(index)[0]) with the
        context rows gathered, normalised and clipped inside the first layer's launch.  train(), or autograd wanted:
        train.DnnIndexedFunction (the staged 16-bit rows are kept for the first layer's weight gradient); eval() without
        autograd: the four inference launches."""
        self._require_device(frames.raw)
        if index.dtype != torch.int32 or index.dim() != 1 or index.numel() == 0 or index.device != frames.raw.device:
            raise ValueError("SpeechEnhancementDNN.forward_indexed: an int32 device index [M] is needed; got %s %s" % (index.dtype, tuple(index.shape)))
        if frames.raw.shape[1] * (2 * frames.context + 1) != self.input_dim:
            raise ValueError("SpeechEnhancementDNN.forward_indexed: frames of %d columns and context %d for rows of %d"
                             % (frames.raw.shape[1], frames.context, self.input_dim))
        index = index.contiguous()
        if self.training or self._wants_autograd(frames.raw):
            from .. import train
            p = float(self.dropout_rate) if self.training else 0.0
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p > 0 else 0
            params = [t for m in self._linears() for t in (m.weight, m.bias)]
            return train.DnnIndexedFunction.apply(frames.raw, frames.bounds, frames.mean_dev, frames.std_dev, index, frames.context, p, seed,
                                                  *params)
        packs = self._packs()
        h = ops.dnn_layer_indexed(frames.raw, frames.bounds, index, packs[0], context=frames.context, act="relu", mean=frames.mean_dev,
                                  std=frames.std_dev)
        return self._tail(h, packs)

    def get_layer_params(self):
        return [(m.weight, m.bias) for m in self._linears()]

    def load_rbm_weights(self, rbm_weights):
        """rbm_weights: (W [visible, hidden], visible_bias, hidden_bias) per hidden layer, numpy arrays or tensors; the output
        layer is never set"""
        linears = self._linears()
        for i, (w, _vb, hb) in enumerate(rbm_weights):
            if i < len(linears) - 1:
                with torch.no_grad():
                    linears[i].weight.copy_(torch.as_tensor(np.asarray(w.detach().cpu() if torch.is_tensor(w) else w)).T)
                    linears[i].bias.copy_(torch.as_tensor(np.asarray(hb.detach().cpu() if torch.is_tensor(hb) else hb)))


def create_dnn(feature_dim, mask_dim=None):
    return SpeechEnhancementDNN(input_dim=feature_dim, hidden_dim=config.DNN_HIDDEN_UNITS, output_dim=mask_dim or config.NUM_CHANNELS,
                                num_hidden_layers=config.DNN_HIDDEN_LAYERS, dropout=config.DNN_DROPOUT)
