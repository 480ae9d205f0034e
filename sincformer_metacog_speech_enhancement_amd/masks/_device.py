"""What the three mirrors share: the argument checks.  Mask functions take fp32 device tensors of one shape and return fp32
device tensors without autograd history (they are targets); a host tensor is refused, there is no CPU fallback."""
import torch


def planes(name, *tensors):
    """the arguments as detached contiguous fp32 device tensors of one shape"""
    out = []
    for t in tensors:
        if not torch.is_tensor(t):
            raise TypeError("%s: device tensors are needed; got %s" % (name, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError("%s: the sincformer HIP path only runs on an MI355X device tensor; got a CPU tensor "
                               "(there is deliberately no CPU fallback)." % name)
        if t.is_complex():
            raise TypeError("%s: a complex tensor is refused (the reference's complex branch does something else and nothing "
                            "calls it); pass magnitudes" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s: fp32 tensors are needed; got %s" % (name, t.dtype))
        if t.shape != tensors[0].shape:
            raise ValueError("%s: shapes differ: %s and %s" % (name, tuple(tensors[0].shape), tuple(t.shape)))
        out.append(t.detach().contiguous())
    if out[0].numel() == 0:
        raise ValueError("%s: empty tensors" % name)
    return out
