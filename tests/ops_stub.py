"""The stub harness of the host tests: ops' wrappers run on CPU tensors against a library that launches nothing, and every
_call is recorded instead of made.  One copy, shared by every *_host.py file that checks launch costs, routing or contracts."""
import torch


class _StubLib:
    """every entry point returns 0; the size helpers (*_floats, *_doubles, *_tiles) return a small positive count, which is also
    a true answer of the predicate sfm_gammatone_tf_fits.  returns: symbol -> another result, for a test that needs one."""

    def __init__(self, returns=None):
        self._returns = dict(returns or {})

    def __getattr__(self, symbol):
        if not symbol.startswith("sfm_"):
            raise AttributeError(symbol)
        rc = self._returns.get(symbol, 4 if symbol.endswith(("_floats", "_doubles", "_tiles", "_fits")) else 0)
        fn = lambda *args: rc
        fn.__name__ = symbol
        return fn


def install(monkeypatch, returns=None, tags=True):
    """patch ops._lib.load, ops._stream, ops._need_dev, ops._call and ops._ws64 for one test -> the list that receives
    (symbol, family, flops, bytes, tag) of every launch the wrappers enqueue (tags=False: without the tag).  The recording
    _call also checks that the argument tuple has the length the header declares."""
    from sincformer_metacog_speech_enhancement_amd import lib, ops
    rec = []
    stub = _StubLib(returns)

    def record(name, fn, args, flops=0.0, nbytes=0.0, tag=None):
        assert len(args) == len(lib.SIGNATURES[fn.__name__]), fn.__name__
        rec.append((fn.__name__, name, flops, nbytes, tag) if tags else (fn.__name__, name, flops, nbytes))

    monkeypatch.setattr(ops._lib, "load", lambda: stub)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_need_dev", lambda *ts: None)
    monkeypatch.setattr(ops, "_call", record)
    monkeypatch.setattr(ops, "_ws64", lambda n, device: torch.zeros(int(n), dtype=torch.float64))
    return rec
