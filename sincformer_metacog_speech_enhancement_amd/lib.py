"""ctypes binding of libsincformer_hip.so, read from the C ABI's one statement: include/sincformer_hip.h.

The product path has NO fallback: if the header, the shared library or a symbol is missing, importing/using the ops raises.
(The oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes
import os
import re

# torch must be imported BEFORE the shared library is dlopen'ed: torch ships its own
# libamdhip64 (same SONAME as the system one).  Loading ours first would pull a second HIP
# runtime into the process and every launch on a torch stream would then fail.
import torch  # noqa: F401  (device memory / stream plumbing; see ops.py)

from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFM_LIB_PATH") or os.path.join(_HERE, "libsincformer_hip.so")   # override: A/B of two builds
HEADER = os.path.join(INCLUDE, "sincformer_hip.h")

_CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "unsigned int": ctypes.c_uint}


def _parse_header(path):
    """(name -> (restype, [argtypes], [parameter names]) of every `sfm_*` function the header declares, in its order;
    name -> int or float of every `#define SFM_<NAME> <literal>` line, without the prefix)"""
    def ctype(text, decl):
        words = [w for w in text.replace("*", " * ").split() if w != "const"]
        if "*" not in words and " ".join(words) not in _CTYPES:
            raise TypeError("%s: no ctypes mapping for %r in `%s`" % (path, text.strip(), " ".join(decl.split())))
        return ctypes.c_void_p if "*" in words else _CTYPES[" ".join(words)]

    with open(path) as f:
        src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    constants = {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+SFM_[^\n]*", src, flags=re.M):      # as loud as the declarations below
        m = re.match(r"\s*#\s*define\s+SFM_(\w+)\s+\(?(-?\d+(\.\d+)?)\)?\s*$", line)
        if m is None or m.group(1) in constants:
            raise SyntaxError("%s: not a (new) `#define SFM_<NAME> <literal>` line: %s" % (path, line.strip()))
        constants[m.group(1)] = float(m.group(2)) if m.group(3) else int(m.group(2))
    n_defines = len(re.findall(r"#\s*define\s+SFM_", src))                    # (one that does not start its line is lost above)
    if n_defines != len(constants):
        raise SyntaxError("%s: %d `#define SFM_` occurrences, %d parsed constants" % (path, n_defines, len(constants)))
    abi = {}
    for m in re.finditer(r"^([^\n;(){}#]*?)\b(sfm_\w+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else [re.match(r"(.*?)(\w*)\s*$", p, flags=re.S) for p in params.split(",")]
        abi[name] = (ctype(ret, m.group(0)), [ctype(p.group(1), m.group(0)) for p in params], [p.group(2) for p in params])
    seen = list(re.finditer(r"sfm_\w+\s*\(", src))     # every mention must be one of the declarations: a lost `;` or a stray brace is loud
    lost = [src[m.start():m.start() + 80].split("\n")[0] for m in seen if m.group(0).rstrip("( \t\n") not in abi]
    if lost or len(seen) != len(abi):
        raise SyntaxError("%s: %d `sfm_*(` occurrences, %d parsed declarations; not parsed: %s" % (path, len(seen), len(abi), lost))
    return abi, constants


ABI, CONSTANTS = _parse_header(HEADER)                                        # CONSTANTS["MIX_CHUNK"] = SFM_MIX_CHUNK
SIGNATURES = {name: argtypes for name, (_, argtypes, _) in ABI.items()}      # name -> argtypes, in the header's order

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes library; raises HipExtensionMissing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipExtensionMissing(
            "libsincformer_hip.so not built (%s). Run `python -m sincformer_metacog_speech_enhancement_amd.build` "
            "or __graft_entry__.build(); there is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes, _) in ABI.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipExtensionMissing("symbol %s missing from %s" % (name, LIB_PATH)) from e
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


_ERR = {CONSTANTS["ERR_ARG"]: "bad argument", CONSTANTS["ERR_SHAPE"]: "unsupported shape", CONSTANTS["ERR_LAUNCH"]: "kernel launch failed"}


def check(rc, name):
    if rc != 0:
        raise RuntimeError("%s failed: %s (%d)" % (name, _ERR.get(rc, "error"), rc))
