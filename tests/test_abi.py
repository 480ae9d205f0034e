"""The C-ABI library loads on a machine without a GPU and exports every symbol that
include/sincformer_hip.h declares, with the parameter and return types the ctypes binding assumes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sincformer_hip.h")


_CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "unsigned int": ctypes.c_uint}


def _ctype(decl):
    """ctypes type of one C parameter or return type, e.g. "const float* x", "unsigned int seed", "long long" """
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    for n in (len(words), len(words) - 1):                  # with or without a parameter name behind the type
        if " ".join(words[:n]) in _CTYPES:
            return _CTYPES[" ".join(words[:n])]
    raise ValueError("no ctypes mapping for %r" % decl)


def _header_decls():
    """name -> (return type, [parameter types]) as ctypes types, for every function the header declares"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(long long|int)\s+(sfm_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        params = [] if args in ("", "void") else [_ctype(a) for a in args.split(",")]
        decls[m.group(2)] = (_ctype(m.group(1)), params)
    return decls


# the entry points that return a size (long long); every other one returns an int status.  Literal: a fault that this file's
# parser and lib's share still fails
RETURNS_LONG_LONG = {
    "sfm_mean_time_scratch_floats", "sfm_sinc_wgrad_scratch_floats", "sfm_sinc_shift_len", "sfm_gn_bwd_reduce_ws_floats",
    "sfm_tn_ws_floats", "sfm_colsum_ws_floats", "sfm_layernorm_bwd_ws_floats", "sfm_col_stats_ws_floats",
    "sfm_dwconv_wgrad_scratch_floats", "sfm_memory_param_floats",
    "sfm_wave_moments_ws_doubles", "sfm_spec_sums_ws_doubles", "sfm_sumsq_ws_doubles", "sfm_memory_bwd_ws_floats",
    "sfm_pstoi_loss_ws_doubles", "sfm_mse_loss_ws_doubles", "sfm_adv_leaky_ws_doubles", "sfm_adv_head_ws_doubles",
    "sfm_adv_head_bwd_ws_floats", "sfm_mix_scale_ws_doubles", "sfm_pso_split_ws_doubles",
}


@pytest.fixture(scope="module")
def built():
    from sincformer_metacog_speech_enhancement_amd import build, lib
    build.build(verbose=False)
    return lib


def test_header_declares_the_bound_symbols(built):
    decls = _header_decls()
    assert len(decls) >= 108                                # (the pattern has not lost a declaration)
    assert set(decls) == set(built.SIGNATURES), set(decls) ^ set(built.SIGNATURES)
    L = built.load()
    for name, (ret, params) in decls.items():
        assert built.SIGNATURES[name] == params, (name, params, built.SIGNATURES[name])
        assert getattr(L, name).restype is ret, (name, ret, getattr(L, name).restype)
    long_long = {name for name, (ret, _) in decls.items() if ret is ctypes.c_longlong}
    assert {name for name, (ret, _, _) in built.ABI.items() if ret is ctypes.c_longlong} == long_long == RETURNS_LONG_LONG


def test_a_surplus_argument_is_refused_before_the_call(built):
    """ctypes passes surplus arguments of a cdecl function through; ops._call compares the tuple with the header first"""
    from sincformer_metacog_speech_enhancement_amd import ops
    L = built.load()
    args = (None, None, None, None, None, 4, 256, 256, 256, 256, 1e-5, 0, 0, None)
    with pytest.raises(RuntimeError, match="bad argument"):             # the right length reaches the library
        ops._call("layernorm", L.sfm_layernorm, args)
    calls = []

    def spy(*a):
        calls.append(a)
        return 0
    spy.argtypes, spy.__name__ = L.sfm_layernorm.argtypes, "sfm_layernorm"
    with pytest.raises(TypeError, match=r"sfm_layernorm takes 14 arguments .* 15 given"):
        ops._call("layernorm", spy, args + (None,))
    assert not calls
    with pytest.raises(TypeError, match="15 given"):
        ops._call("layernorm", L.sfm_layernorm, args + (None,))


def test_a_wrongly_typed_argument_is_named_as_in_the_header(built):
    from sincformer_metacog_speech_enhancement_amd import ops
    L = built.load()
    with pytest.raises(ctypes.ArgumentError, match=r"sfm_layernorm, parameter `ldx`"):
        ops._call("layernorm", L.sfm_layernorm, (None, None, None, None, None, 4, 256, "256", 256, 256, 1e-5, 0, 0, None))


def test_library_exports_every_symbol(built):
    L = built.load()
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in _header_decls():
        assert hasattr(raw, name), name
    assert L.sfm_abi_version() == 1


def test_missing_library_is_loud(monkeypatch, built):
    monkeypatch.setattr(built, "_lib", None)
    monkeypatch.setattr(built, "LIB_PATH", "/nonexistent/libsincformer_hip.so")
    with pytest.raises(built.HipExtensionMissing):
        built.load()


def test_null_pointers_are_rejected_without_a_gpu(built):
    """argument validation happens before any HIP call, so it can be exercised on CPU"""
    L = built.load()
    assert L.sfm_attention_fwd(None, None, 1, 1, 1, 64, 192, 64, 64, 128, 192, 64, 0.125, 0, None) == -1
    assert L.sfm_layernorm(None, None, None, None, None, 4, 256, 256, 256, 256, 1e-5, 0, 0, None) == -1
    one = ctypes.c_void_p(16)
    assert L.sfm_gemm16(one, one, None, one, None, None, 1, 8, 8, 12, 12, 1, 1, 0, 0, 32, 8, 64, 8, 0, 0, 0, 1.0, 0, 1,
                        0, 0, 0, None) == -2       # Cin not a multiple of 8
    assert L.sfm_bilstm_layer(one, one, one, 2, 5, 100, 0, None) == -2   # unsupported hidden size
    assert L.sfm_bilstm_layer_ex(one, one, one, 2, 5, 100, 1, None) == -2


def test_layernorm_row_strides_narrower_than_the_row_are_rejected_without_a_gpu(built):
    """sfm_layernorm / sfm_layernorm_bwd_ex / sfm_layernorm_bwd_next refuse (SFM_ERR_SHAPE) a row stride below D: rows would
    overlap and the last one would run past its buffer.  Every call carries an invalid dtype, checked after the shapes: the
    controls pass every stride check and are then refused for it (SFM_ERR_ARG), and no call here can reach a launch."""
    L = built.load()
    one = ctypes.c_void_p(16)
    M, D, BAD_DT = 4, 384, 7
    # forward: x, out16, out32 strides
    assert L.sfm_layernorm(one, one, one, one, None, M, D, D, D, 0, 1e-5, 0, BAD_DT, None) == -1           # control
    assert L.sfm_layernorm(one, one, one, one, one, M, D, D + 8, D, D + 4, 1e-5, 0, BAD_DT, None) == -1   # control, wide strides
    assert L.sfm_layernorm(one, one, one, None, one, M, D, 512, 0, 512, 1e-5, 0, BAD_DT, None) == -1      # control: no out16
    assert L.sfm_layernorm(one, one, one, one, None, M, D, 256, D, 0, 1e-5, 0, BAD_DT, None) == -2        # ldx < D
    assert L.sfm_layernorm(one, one, one, one, None, M, D, D, 256, 0, 1e-5, 0, BAD_DT, None) == -2        # ld16 < D
    assert L.sfm_layernorm(one, one, one, None, one, M, D, D, 0, 256, 1e-5, 0, BAD_DT, None) == -2        # ld32 < D
    assert L.sfm_layernorm(one, one, one, one, one, M, D, D, D, D - 1, 1e-5, 0, BAD_DT, None) == -2
    assert L.sfm_layernorm(one, one, one, one, None, M, 513, 513, 513, 0, 1e-5, 0, BAD_DT, None) == -2    # D > 512
    # backward: ldx, ldy, ld (dres / dx)
    for fn, tail in ((L.sfm_layernorm_bwd_ex, ()), (L.sfm_layernorm_bwd_next, (one, 1.0, 0.0, 0))):
        def call(ldx, ldy, ld, dt):
            args = (one, one, one, 0, one, one, one, one, M, D, ldx, ldy, ld, 1e-5, dt) + tail + (None, None)
            return fn(*args)
        assert call(D, D, D, BAD_DT) == -1                                                                   # control
        assert call(D + 16, D + 8, D + 4, BAD_DT) == -1                                                      # control
        assert call(256, D, D, BAD_DT) == -2
        assert call(D, 256, D, BAD_DT) == -2
        assert call(D, D, 256, BAD_DT) == -2


def test_depthwise_conv_shape_checks_without_a_gpu(built):
    """sfm_dwconv_folded takes any C > 0 and odd KS (generic kernel beside the register-resident ones); C <= 0 and even KS are
    refused before any launch (C = 0 used to divide by zero in the check itself)"""
    L = built.load()
    one = ctypes.c_void_p(16)
    assert L.sfm_dwconv_folded(one, one, one, one, one, 2, 10, 0, 7, 1, 0, 7, None) == -2
    assert L.sfm_dwconv_folded(one, one, one, one, one, 2, 10, 192, 8, 1, 0, 7, None) == -2
    assert L.sfm_dwconv_folded(one, one, one, one, one, 2, 10, 192, 15, 1, 0, 7, None) == -1     # control: shape accepted
    assert L.sfm_dwconv_folded(one, one, one, one, one, 2, 10, 256, 31, 1, 0, 7, None) == -1


def test_time_reductions_refuse_a_row_stride_below_the_row_without_a_gpu(built):
    """sfm_sum_time / sfm_mean_time read C columns of rows ld_src apart: ld_src < C (rows overlap, the last one runs past its
    buffer) is SFM_ERR_SHAPE, returned before any launch"""
    L = built.load()
    one = ctypes.c_void_p(16)
    assert L.sfm_sum_time(one, one, one, 2, 5, 129, 128, None) == -2
    assert L.sfm_mean_time(one, one, one, 2, 5, 129, 128, None) == -2
    assert L.sfm_sum_time(one, one, one, 2, 5, 129, 0, None) == -2
    assert L.sfm_mean_time(one, one, None, 2, 5, 129, 136, None) == -1      # (a null pointer is refused first, as everywhere)
    assert L.sfm_sum_time(one, one, None, 2, 5, 129, 129, None) == -1


# ---- the shared constants: include/sincformer_hip.h states them, lib.CONSTANTS reads them, ops re-exports them ----------------
def test_constants_hold_every_define_of_the_header(built):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"#\s*define\s+SFM_(\w+)", src)
    assert len(names) >= 50 and len(set(names)) == len(names)
    assert sorted(names) == sorted(built.CONSTANTS)
    for name, value in built.CONSTANTS.items():
        assert type(value) in (int, float), (name, value)
    assert built._ERR == {-1: "bad argument", -2: "unsupported shape", -3: "kernel launch failed"}


# what ops.py (and lib._ERR, ops._DT_ID) stated as literals before the header became their one statement: no value changed
OPS_CONSTANTS = {
    "EPI_NONE": 0, "EPI_SWISH": 1, "EPI_GELU": 2, "EPI_RESID": 3, "EPI_GLU": 4, "EPI_SIGMOID": 5, "EPI_TANH_SCALE": 6,
    "EPI_SIGMA": 7, "EPI_CPEA": 8,
    "LAYERNORM_MAX_D": 512, "ATTN_QTILE": 128, "DWCONV_TILE": 64, "_XCDS": 8, "_XCD_RUN": 8,
    "MIX_CHUNK": 4096, "QUANT_MAX_STEPS": 16, "PSO_CHUNK": 4096, "PSO_FRAMES": 8, "PSO_MAX_PARTICLES": 256, "PSO_MAX_BINS": 1024,
    "GT_COLS": 64, "GT_ROWS": 384, "GT_MAX_TAPS": 2048, "GT_LDS_MAX": 160 * 1024,
    "FE_MAX_FILTERS": 64, "FE_MAX_BINS": 257, "FE_MAX_COEFFS": 16,
    "CEP_POWER": 0, "CEP_MAGNITUDE": 1, "CEP_BLOCKS": 2, "CEP_NONE": 0, "CEP_LOG": 1, "CEP_CBRT": 2,
    "HC_PARAMS": 12, "ADV_MAX_WIDTH": 512, "ADV_LO_SCALE": 2048.0, "CSII_BINS": 129, "HE_ROWS": 256, "HE_KSTEP": 64,
    "DNN_ROW_TILE": 128, "DNN_CONTEXT_MAX_K": 4096,
    "MASK_KINDS": {None: 0, "irm": 1, "pcirm": 2, "opt_pcirm": 3}, "DNN_ACT": {None: 0, "relu": 1, "sigmoid": 2},
    # the limits of sfm_pstoi_loss, bare numbers in the wrapper's check until now
    "PSTOI_MAX_BANDS": 32, "PSTOI_MAX_BINS": 257, "PSTOI_MIN_FRAME_LEN": 2, "PSTOI_MAX_FRAME_LEN": 32,
    # Python-only constants stay literals
    "HC_STEP_FLOPS": 24.0, "HILBERT_TAB_CACHE": 1024, "ATTN_QSCALE_LOG2E": 1.4426950408889634,
}


def test_no_shared_constant_changed_value(built):
    import torch
    from sincformer_metacog_speech_enhancement_amd import ops
    for name, value in OPS_CONSTANTS.items():
        got = getattr(ops, name)
        assert got == value and type(got) is type(value), (name, got, value)
    assert ops._DT_ID == {torch.bfloat16: 0, torch.float16: 1}
    assert built.CONSTANTS["SINC_FIR16_WS_WORDS"] == 8 * 2 * 64 * 272
    assert (built.CONSTANTS["OK"], built.CONSTANTS["ERR_ARG"], built.CONSTANTS["ERR_SHAPE"], built.CONSTANTS["ERR_LAUNCH"]) == (0, -1, -2, -3)


@pytest.mark.parametrize("bad", ["#define SFM_X", "#define SFM_X 160 * 1024", "#define SFM_X (1 << 4)", "#define SFM_X abc",
                                 "  #define SFM_OK 1"])
def test_a_malformed_define_fails_the_parse_with_its_line(built, tmp_path, bad):
    """on a scratch copy of the header: a `#define SFM_` line that is no plain literal (or states a name twice) is as loud as a
    declaration the parser cannot read"""
    text = open(HEADER).read()
    marker = "int sfm_abi_version(void);"
    assert marker in text
    scratch = tmp_path / "sincformer_hip.h"
    scratch.write_text(text)
    abi, constants = built._parse_header(str(scratch))                  # control: the copy itself parses
    assert abi.keys() == built.ABI.keys() and constants == built.CONSTANTS
    scratch.write_text(text.replace(marker, bad + "\n" + marker))
    with pytest.raises(SyntaxError) as e:
        built._parse_header(str(scratch))
    assert bad.strip() in str(e.value)


def test_scratch_size_queries_without_a_gpu(built):
    """every workspace is sized by the library; the expected values are the formulas the wrappers used to carry, as literals"""
    L = built.load()
    assert L.sfm_wave_moments_ws_doubles(3, 257) == 64 * 3 * 5 == 960            # the block cap, whatever L
    assert L.sfm_wave_moments_ws_doubles(3, 16385) == 960
    assert L.sfm_wave_moments_ws_doubles(1, 1) == 320
    assert L.sfm_spec_sums_ws_doubles(257) == 2048 * 4 == 8192
    assert L.sfm_spec_sums_ws_doubles(2048 * 256 + 1) == 8192
    assert L.sfm_sumsq_ws_doubles(1) == 2048
    assert L.sfm_sumsq_ws_doubles(2048 * 256 + 1) == 2048
    assert L.sfm_mse_loss_ws_doubles(1025) == 1025
    assert L.sfm_mse_loss_ws_doubles(1024 * 1024 + 1) == 1025
    assert L.sfm_pstoi_loss_ws_doubles(2, 61, 30) == 2 * 2 + 1 == 5               # B * (T // frame_len) + 1
    assert L.sfm_pstoi_loss_ws_doubles(3, 30, 30) == 4
    assert L.sfm_pstoi_loss_ws_doubles(1, 100, 7) == 15
    assert L.sfm_mix_scale_ws_doubles(2, 4097) == 8                               # 2 * B * ceil(L / 4096)
    assert L.sfm_mix_scale_ws_doubles(2, 4096) == 4
    assert L.sfm_mix_scale_ws_doubles(3, 1) == 6
    assert L.sfm_pso_split_ws_doubles(2, 4097) == 16                              # 4 * B * ceil(Lmax / 4096)
    assert L.sfm_pso_split_ws_doubles(1, 4096) == 4
    assert L.sfm_pso_split_ws_doubles(5, 12289) == 80
    assert L.sfm_adv_leaky_ws_doubles(4) == 2048
    assert L.sfm_adv_leaky_ws_doubles(4 * 256 * 2048 + 4) == 2048
    assert L.sfm_adv_head_ws_doubles(1, 5) == 2                                   # ceil(B T / 4)
    assert L.sfm_adv_head_ws_doubles(2, 4) == 2
    assert L.sfm_adv_head_ws_doubles(3, 7) == 6
    assert L.sfm_adv_head_bwd_ws_floats(1, 65, 8) == 50                           # ceil(B T / 64) * (3 C + 1)
    assert L.sfm_adv_head_bwd_ws_floats(1, 64, 8) == 25
    assert L.sfm_adv_head_bwd_ws_floats(2, 100, 32) == 4 * 97
    npar = L.sfm_memory_param_floats(8, 4, 3)                                     # Bn * npar
    assert npar == 2 * 64 + 32 + 24 + 12 + 16 + 4 + 8 + 4 + 1 == 229
    assert L.sfm_memory_bwd_ws_floats(2, 8, 4, 3) == 458
    assert L.sfm_memory_bwd_ws_floats(1, 8, 4, 3) == 229


def _gammatone_tf_fits_rule(K, hop):
    """ops.gammatone_tf_fits as it stood while it restated the kernel's LDS layout"""
    GT_COLS, GT_ROWS, GT_MAX_TAPS, GT_LDS_MAX = 64, 384, 2048, 160 * 1024
    lds = 4 * (GT_ROWS + K + GT_ROWS * 65 + 2 * hop * GT_COLS)
    return 8 <= K <= GT_MAX_TAPS and K % 8 == 0 and 2 <= hop <= GT_ROWS and hop % 2 == 0 and lds <= GT_LDS_MAX


def test_gammatone_tf_fits_is_the_rule_the_wrapper_restated(built):
    from sincformer_metacog_speech_enhancement_amd import ops
    L = built.load()
    # 4 (384 + K + 384 * 65 + 128 hop) <= 163840 at K 2048: hop <= 106.5
    assert _gammatone_tf_fits_rule(2048, 106) and not _gammatone_tf_fits_rule(2048, 108)
    grid = [(K, hop) for K in (0, 8, 12, 16, 800, 2048, 2056) for hop in (0, 1, 2, 3, 106, 108, 128, 384, 386)]
    assert any(_gammatone_tf_fits_rule(K, hop) for K, hop in grid) and not all(_gammatone_tf_fits_rule(K, hop) for K, hop in grid)
    for K, hop in grid:
        assert bool(L.sfm_gammatone_tf_fits(K, hop)) == _gammatone_tf_fits_rule(K, hop), (K, hop)
        assert ops.gammatone_tf_fits(K, hop) is _gammatone_tf_fits_rule(K, hop), (K, hop)
