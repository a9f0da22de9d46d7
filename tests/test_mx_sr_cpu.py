"""CPU tier of MX fake quantization with stochastic rounding: the generator's known answers, the fqs_ header and
its binding, every refusal of the two launching entry points in the order the header states (validation precedes every HIP call, so no GPU
is needed: the non-NULL pointers below are never dereferenced), the Python argument checks, QuantizeLinear's constructor rules, and the
properties of the numpy reference itself (tests/mx_sr_reference.py) -- fixed points, neighbours, determinism and unbiasedness."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_reference as M
import mx_rules_reference as R
import mx_sr_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0x1000, 0x2000                      # 16-byte aligned, never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
E4M3, CEIL, ROTATE = 3, 2, 1
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 11008, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]
U64 = 2 ** 64 - 1
FMTS = list(M.FORMATS)


def call(name, x, y, rows, cols, fmt, dtype, flags, seed=0, stream_id=0):
    L = _lib.lib()
    rc = getattr(L, name)(x, y, rows, cols, fmt, dtype, flags, seed, stream_id, None)
    return rc, L.fq_last_error().decode()


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in S.philox4x32_10([counter], key)[0]) == want


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_the_library_draws_the_same_words(counter, key, want):
    """fqs_mx_noise runs, on the host, the function the kernels call: the eight R16 of counter c are the four words, low half first"""
    seed, stream_id, c = key[0] | key[1] << 32, counter[2] | counter[3] << 32, counter[0] | counter[1] << 32
    if c << 3 > 2 ** 63 - 9:
        c &= 2 ** 59 - 1                   # the flat index is an int64: the largest counter a tensor can reach
        want = tuple(int(w) for w in S.philox4x32_10([(c & 0xFFFFFFFF, c >> 32, counter[2], counter[3])], key)[0])
    out = (ctypes.c_uint16 * 8)()
    for dtype in (BF16, F16, F32):         # the words do not depend on the vector's width
        assert _lib.lib().fqs_mx_noise(seed, stream_id, c << 3, 8, dtype, out) == 0
        assert [out[2 * k] | out[2 * k + 1] << 16 for k in range(4)] == list(want)


def test_the_noise_index_is_64_bit():
    """flat indices beyond 2^32 and 2^35 (counter word 1 not zero), unaligned starts, both vector widths, against the numpy generator"""
    L = _lib.lib()
    out = (ctypes.c_uint16 * 100)()
    for seed, stream_id in ((0, 0), (U64, U64), (0x0123456789ABCDEF, 0xFEDCBA9876543210)):
        for first in (0, 3, 2 ** 32 - 7, 2 ** 35 - 50, 2 ** 35 + 1, 2 ** 47 + 5, 2 ** 63 - 101):
            for dtype in (BF16, F32):
                assert L.fqs_mx_noise(seed, stream_id, first, 100, dtype, out) == 0
                assert np.array_equal(np.array(out[:], dtype=np.uint16), S.r16(seed, stream_id, np.arange(first, first + 100, dtype=np.uint64)))
    assert L.fqs_mx_noise(0, 0, -1, 4, BF16, out) == SHAPE and L.fqs_mx_noise(0, 0, 0, 2 ** 24 + 1, BF16, out) == SHAPE
    assert L.fqs_mx_noise(0, 0, 2 ** 63 - 1, 2, BF16, out) == SHAPE and L.fqs_mx_noise(0, 0, 0, 4, F64, out) == DTYPE
    assert L.fqs_mx_noise(0, 0, 0, 4, BF16, None) == NULL and L.fqs_mx_noise(0, 0, 5, 0, BF16, None) == 0


# ---- header and binding ------------------------------------------------------------------------------------------------------------------------

def test_sr_header_names_equal_sr_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_sr.h")).read()
    assert '#include "llmqat_fakequant.h"' in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqs_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.SR_EXPORTS) >= {"fqs_mx_fwd", "fqs_mx_fwd_cols"}
    assert not re.findall(r"\bfq_[a-z0-9_]+\s*\(", src) and not re.findall(r"\bfqt_[a-z0-9_]+\s*\(", src)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert not set(_lib.SR_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS))
    assert set(_lib.TRAIN_EXPORTS) == {"fqt_mx_fwd_cols"}
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64
    for name in ("fqs_mx_fwd", "fqs_mx_fwd_cols"):
        f = getattr(L, name)
        assert f.argtypes == [vp, vp, i64, i64, i32, i32, i32, u64, u64, vp] and f.restype is i32
    assert L.fqs_mx_noise.argtypes == [u64, u64, i64, i64, i32, vp] and L.fqs_mx_noise.restype is i32


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

HEAD = [
    # (x, y, rows, cols, fmt, dtype, flags), code, part of the message: the same for both entry points
    ((None, None, -1, -1, 9, 9, 4), DTYPE, "unknown dtype"),
    ((None, None, -1, -1, 9, -1, 4), DTYPE, "unknown dtype"),
    ((None, None, -1, -1, 9, F64, 4), DTYPE, "float64"),
    ((None, None, -1, -1, 5, BF16, 4), ARG, "unknown MX format"),
    ((None, None, -1, -1, -1, F32, 4), ARG, "unknown MX format"),
    ((None, None, -1, -1, E4M3, BF16, 4), ARG, "flag bits 0x4"),
    ((None, None, -1, -1, E4M3, BF16, ROTATE), ARG, "flag bits 0x1"),
    ((None, None, -1, -1, E4M3, F16, CEIL | ROTATE), ARG, "flag bits 0x1"),
]
COLS_REFUSALS = HEAD + [
    ((None, None, -32, 8, E4M3, BF16, 0), SHAPE, "negative shape"),
    ((None, None, 33, -1, E4M3, BF16, CEIL), SHAPE, "negative shape"),
    ((None, None, 33, 8, E4M3, BF16, 0), SHAPE, "rows=33 is not a multiple of the 32"),
    ((None, None, 31, 0, E4M3, F32, 0), SHAPE, "not a multiple"),                     # rows % 32 comes before the empty shape
    ((None, None, 2 ** 62, 2 ** 40, E4M3, BF16, 0), SHAPE, "overflows"),
    ((None, B, 32, 8, E4M3, BF16, 0), NULL, "NULL"),
    ((A, None, 32, 8, E4M3, BF16, 0), NULL, "NULL"),
    ((None, None, 32, 3, E4M3, BF16, 0), NULL, "NULL"),
    ((A + 2, A + 2, 32, 3, E4M3, BF16, 0), ARG, "in-place"),                          # y == x comes before the alignment
    ((A + 2, B, 32, 3, E4M3, BF16, 0), UNSUPPORTED, "16-byte aligned"),
    ((A, B + 8, 32, 3, E4M3, F32, CEIL), UNSUPPORTED, "16-byte aligned"),
    ((A, B, 2 ** 36, 4, E4M3, BF16, 0), UNSUPPORTED, "whole 16-byte vectors"),        # the row's bytes come before the grid
    ((A, B, 32, 7, E4M3, F16, 0), UNSUPPORTED, "whole 16-byte vectors"),
    ((A, B, 32, 6, E4M3, F32, 0), UNSUPPORTED, "whole 16-byte vectors"),
    ((A, B, 2 ** 36, 8, E4M3, BF16, 0), UNSUPPORTED, "exceed one launch's grid"),     # 2^31 row tiles
    ((A, B, 2 ** 35, 8 * 65, E4M3, BF16, CEIL), UNSUPPORTED, "exceed one launch's grid"),   # 2^30 row tiles x 2 column tiles
]
ROWS_REFUSALS = HEAD + [
    ((None, None, -1, 31, E4M3, BF16, 0), SHAPE, "negative shape"),
    ((None, None, 3, -32, E4M3, BF16, CEIL), SHAPE, "negative shape"),
    ((None, None, 2 ** 62, 33, E4M3, BF16, 0), SHAPE, "cols=33 is not a multiple of the 32"),   # cols % 32 comes before the overflow
    ((None, None, 0, 31, E4M3, F32, 0), SHAPE, "not a multiple"),                     # ... and before the empty shape
    ((None, None, 2 ** 40, 2 ** 40, E4M3, BF16, 0), SHAPE, "overflows"),
    ((None, B, 3, 32, E4M3, BF16, 0), NULL, "NULL"),
    ((A, None, 3, 32, E4M3, BF16, 0), NULL, "NULL"),
    ((A + 2, A + 2, 3, 32, E4M3, BF16, 0), ARG, "in-place"),                          # y == x comes before the alignment
    ((A + 2, B, 3, 32, E4M3, BF16, 0), UNSUPPORTED, "16-byte aligned"),
    ((A, B + 8, 3, 32, E4M3, F32, CEIL), UNSUPPORTED, "16-byte aligned"),
    ((A, B, 2 ** 45, 2 ** 14, E4M3, BF16, 0), UNSUPPORTED, "exceed one launch's grid"),     # 2^59 elements: 2^56 vectors
]


@pytest.mark.parametrize("args, code, text", COLS_REFUSALS)
def test_every_refusal_of_the_column_entry_point_in_the_stated_order(args, code, text):
    rc, msg = call("fqs_mx_fwd_cols", *args, seed=U64, stream_id=7)
    assert rc == code, (rc, msg)
    assert text in msg, msg
    L = _lib.lib()                           # ... which is fqt_mx_fwd_cols's answer to the same arguments
    assert L.fqt_mx_fwd_cols(*args, None) == code and text in L.fq_last_error().decode()


@pytest.mark.parametrize("args, code, text", ROWS_REFUSALS)
def test_every_refusal_of_the_row_entry_point_in_the_stated_order(args, code, text):
    rc, msg = call("fqs_mx_fwd", *args, seed=3, stream_id=U64)
    assert rc == code, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("name, rows, cols", [("fqs_mx_fwd", 3, 32), ("fqs_mx_fwd_cols", 32, 8)])
def test_every_format_dtype_seed_and_stream_passes_the_first_checks(name, rows, cols):
    for fmt in range(5):
        for dtype in (F32, BF16, F16):
            for flags in (0, CEIL):
                for seed, stream_id in ((0, 0), (U64, U64), (2 ** 63, 1)):
                    assert call(name, None, None, rows, cols, fmt, dtype, flags, seed, stream_id)[0] == NULL      # the pointers are next


def test_empty_shapes_return_zero_without_a_launch():
    for rows, cols in ((0, 8), (32, 0), (0, 0), (0, 3), (64, 0)):
        rc, msg = call("fqs_mx_fwd_cols", None, None, rows, cols, E4M3, BF16, 0)
        assert rc == 0 and msg == "", (rows, cols, rc, msg)
    for rows, cols in ((0, 32), (5, 0), (0, 0), (0, 64)):
        rc, msg = call("fqs_mx_fwd", None, None, rows, cols, E4M3, BF16, CEIL, 9, 9)
        assert rc == 0 and msg == "", (rows, cols, rc, msg)


@pytest.mark.parametrize("name", ["fqs_mx_fwd", "fqs_mx_fwd_cols"])
def test_fuzz_never_reaches_a_launch(name):
    rng = random.Random(19)
    L = _lib.lib()
    f = getattr(L, name)
    block_ok = (lambda rows, cols: cols % 32 == 0) if name == "fqs_mx_fwd" else (lambda rows, cols: rows % 32 == 0)
    seen = set()
    for _ in range(400):
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        fmt, dtype, flags = (max(-(2 ** 31), min(2 ** 31 - 1, rng.choice(INTS))) for _ in range(3))
        rc = f(None, None, rows, cols, fmt, dtype, flags, rng.getrandbits(64), rng.getrandbits(64), None)
        assert rc in (0, DTYPE, ARG, SHAPE, NULL), (rc, rows, cols, fmt, dtype, flags)
        assert rc != 0 or rows == 0 or cols == 0
        assert rc != 0 or L.fq_last_error() == b""
        seen.add(rc)
    assert {DTYPE, ARG} <= seen
    # the same hostile sizes behind valid codes, so that the shape checks are the ones that answer
    for _ in range(400):
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        rc = f(None, None, rows, cols, rng.randrange(5), rng.randrange(3), rng.choice((0, CEIL)), rng.getrandbits(64), rng.getrandbits(64), None)
        assert rc in (0, SHAPE, NULL), (rc, rows, cols)
        assert (rc == 0) == (rows >= 0 and cols >= 0 and block_ok(rows, cols) and (rows == 0 or cols == 0)), (rc, rows, cols)


# ---- Python front-end (all checks before the device check, so CPU tensors reach them) ----------------------------------------------------------

@pytest.mark.parametrize("f", [ops.mx_quantize_sr, llm_qat_amd.mx_quantize_sr])
def test_python_value_errors(f):
    x = torch.zeros(2, 64, 64)
    for bad in (-1, 2 ** 64, 1.0, None, "7", True, False, torch.tensor(3)):
        with pytest.raises(ValueError, match="seed must be a Python int"):
            f(x, "mxfp4", bad)
        with pytest.raises(ValueError, match="stream must be a Python int"):
            f(x, "mxfp4", 1, bad)
    for axis in (0, -3, 3, 1.0, None, True):
        with pytest.raises(ValueError, match="axis"):
            f(x, "mxfp4", 1, axis=axis)
    with pytest.raises(ValueError, match="unknown MX format"):
        f(x, "mxfp5", 1)
    with pytest.raises(ValueError, match="scale_rule"):
        f(x, "mxfp4", 1, scale_rule="up")
    with pytest.raises(ValueError, match="last dimension"):
        f(torch.zeros(2, 64, 48), "mxfp4", 1)
    with pytest.raises(ValueError, match="multiple of 32"):
        f(torch.zeros(2, 48, 64), "mxfp4", 1, axis=-2)
    with pytest.raises(ValueError, match="at least two dimensions"):
        f(torch.zeros(64), "mxfp4", 1, axis=-2)
    with pytest.raises(ValueError, match="whole 16-byte vectors"):
        f(torch.zeros(64, 6), "mxfp4", 1, axis=-2)                     # fp32: 4 elements per vector
    with pytest.raises(ValueError, match="whole 16-byte vectors"):
        f(torch.zeros(64, 12, dtype=torch.bfloat16), "mxfp4", 1, axis=0)   # axis 0 of a matrix is axis -2
    for kw in (dict(), dict(axis=-2), dict(stream=U64, scale_rule="ceil", axis=1)):      # the arguments are fine: what is left is the device
        with pytest.raises(RuntimeError, match="no CPU"):
            f(x, "mxfp4", U64, **kw)
    with pytest.raises(TypeError, match="torch.Tensor"):
        f([1.0] * 32, "mxfp4", 1)


def test_signatures_of_the_new_functions():
    want = [("x", inspect._empty), ("fmt", inspect._empty), ("seed", inspect._empty), ("stream", 0), ("scale_rule", "floor"), ("axis", -1)]
    for f in (ops.mx_quantize_sr, llm_qat_amd.mx_quantize_sr):
        assert [(n, p.default) for n, p in inspect.signature(f).parameters.items()] == want
    assert list(inspect.signature(llm_qat_amd.mx_sr_seed).parameters) == ["seed"]
    assert list(inspect.signature(llm_qat_amd.default_mx_backward_rounding).parameters) == ["mode"]
    assert inspect.signature(QuantizeLinear.__init__).parameters["mx_backward_rounding"].default is None
    for name in ("mx_quantize_sr", "mx_sr_seed", "default_mx_backward_rounding"):
        assert name in llm_qat_amd.__all__
    for k in ("mx_sr_launch", "mx_sr_cols_launch"):
        assert k in ops.mx_counts


def test_not_served_while_compiling():
    def f(x):
        return llm_qat_amd.mx_quantize_sr(x, "mxfp4", 1)
    with pytest.raises(Exception, match="not served while torch.compile traces"):
        torch.compile(f, fullgraph=True, backend="eager")(torch.zeros(4, 32))


def test_mx_sr_seed_returns_the_previous_seed():
    first = llm_qat_amd.mx_sr_seed(11)
    try:
        assert llm_qat_amd.mx_sr_seed(U64) == 11 and llm_qat_amd.mx_sr_seed(0) == U64
        for bad in (-1, 2 ** 64, 1.5, None, True):
            with pytest.raises(ValueError, match="seed must be a Python int"):
                llm_qat_amd.mx_sr_seed(bad)
        assert llm_qat_amd.mx_sr_seed(5) == 0
    finally:
        from llm_qat_amd import utils_quant
        utils_quant._sr_state.update(seed=first, next=0)


MX = dict(w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3")


def test_constructor_rules_of_mx_backward_rounding():
    for mode in ("nearest", "stochastic"):
        assert QuantizeLinear(128, 96, mx_backward_format="mxfp4", mx_backward_rounding=mode, **MX).mx_backward_rounding == mode
    assert QuantizeLinear(128, 96, mx_backward_format="mxfp4", **MX).mx_backward_rounding is None
    with pytest.raises(ValueError, match="no mx_backward_format"):
        QuantizeLinear(128, 96, mx_backward_rounding="stochastic", **MX)
    with pytest.raises(ValueError, match="no mx_backward_format"):
        QuantizeLinear(128, 96, w_bits=4, a_bits=8, mx_backward_rounding="nearest")
    for bad in ("random", "Stochastic", 1, True):
        with pytest.raises(ValueError, match="unknown rounding"):
            QuantizeLinear(128, 96, mx_backward_format="mxfp4", mx_backward_rounding=bad, **MX)
    m = QuantizeLinear(128, 96, mx_backward_format="mxfp4", mx_backward_rounding="stochastic", **MX)
    assert set(m.state_dict()) == set(QuantizeLinear(128, 96, **MX).state_dict()) == {"weight"}
    assert "mx_backward_rounding" not in QuantizeLinear(128, 96, **MX).__dict__          # a class attribute where it is not set
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 128))


def test_process_default_applies_only_to_layers_with_a_backward_format():
    assert llm_qat_amd.default_mx_backward_rounding("stochastic") is None
    try:
        assert QuantizeLinear(128, 96, mx_backward_format="mxfp4", **MX).mx_backward_rounding == "stochastic"
        assert QuantizeLinear(128, 96, mx_backward_format="mxfp4", mx_backward_rounding="nearest", **MX).mx_backward_rounding == "nearest"    # explicit wins
        assert QuantizeLinear(128, 96, **MX).mx_backward_rounding is None                                   # no backward format
        assert QuantizeLinear(128, 96, w_bits=4, a_bits=8).mx_backward_rounding is None
        llm_qat_amd.default_mx_backward_format("mxfp8_e4m3")
        try:
            m = QuantizeLinear(128, 96, **MX)                                                               # both defaults
            assert (m.mx_backward_format, m.mx_backward_rounding) == ("mxfp8_e4m3", "stochastic")
            assert QuantizeLinear(128, 96, mx_backward_rounding="nearest", **MX).mx_backward_rounding == "nearest"     # a default format is in force
            assert QuantizeLinear(128, 48, **MX).mx_backward_rounding is None                               # out % 32: no backward format
        finally:
            llm_qat_amd.default_mx_backward_format(None)
        with pytest.raises(ValueError, match="unknown rounding"):
            llm_qat_amd.default_mx_backward_rounding("up")
        assert llm_qat_amd.default_mx_backward_rounding("nearest") == "stochastic"                          # -> the previous one
    finally:
        llm_qat_amd.default_mx_backward_rounding(None)
    assert llm_qat_amd.default_mx_backward_rounding(None) is None
    assert QuantizeLinear(128, 96, mx_backward_format="mxfp4", **MX).mx_backward_rounding is None


# ---- properties of the reference itself ----------------------------------------------------------------------------------------------------------

def grid_bits(dtype, fmt, rng, blocks=8):
    """blocks whose every element is on the block's grid: max-normal as amax, the rest drawn from the format's code table"""
    table = M.code_table(fmt)
    v = rng.choice(table, (blocks, 32)) * rng.choice([-1.0, 1.0], (blocks, 32))
    v[:, 0] = table[-1]
    return M.encode(v * np.exp2(rng.integers(-6, 6, (blocks, 1)).astype(np.float64)), dtype)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_grid_values_are_fixed_points_for_64_seeds(dtype, fmt):
    rng = np.random.default_rng(1)
    b = grid_bits(dtype, fmt, rng)
    for rule in R.RULES:
        for seed in range(64):
            assert np.array_equal(S.quantize_bits(b, dtype, fmt, rule, seed * 0x9E3779B97F4A7C15 & U64, seed), b)


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_output_is_a_grid_neighbour(fmt, rule):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((64, 64)) * np.exp2(rng.integers(-10, 10, (64, 2)).repeat(32, axis=1).astype(np.float64))
    b = M.encode(x, "fp32")
    for axis in (-1, -2):
        p = S.parts(b, "fp32", fmt, rule, 5, 6, axis)
        ax = np.abs(p["x"])
        assert (p["lo"] <= p["hi"]).all() and (np.abs(p["y"]) == np.where(p["up"], p["hi"], p["lo"])).all()
        clipped = ax > p["hi"]                                    # only the saturated top binade of the floor rule lies outside its neighbours
        assert (p["lo"] <= ax)[~clipped].all()
        assert not clipped.any() if rule == "ceil" else (p["hi"][clipped] == p["lo"][clipped]).all()
        assert (np.abs(p["y"])[p["lo"] == ax] == ax[p["lo"] == ax]).all()         # on the grid: never up
        assert p["up"].any() and not p["up"].all()
        assert (np.signbit(p["y"]) == np.signbit(p["x"])).all()


def test_same_seed_and_stream_same_bits_and_any_other_differs():
    rng = np.random.default_rng(3)
    b = M.encode(rng.standard_normal(4096), "bf16")
    base = S.quantize_bits(b, "bf16", "mxfp4", "floor", 7, 9)
    assert np.array_equal(base, S.quantize_bits(b.copy(), "bf16", "mxfp4", "floor", 7, 9))
    for seed, stream in ((8, 9), (7, 10), (7 | 1 << 32, 9), (7, 9 | 1 << 32), (9, 7)):
        assert not np.array_equal(base, S.quantize_bits(b, "bf16", "mxfp4", "floor", seed, stream)), (seed, stream)
    assert not np.array_equal(base, S.quantize_bits(b, "bf16", "mxfp4", "floor", 7, 9, first=8))        # ... and another place in the tensor


def unbiased_block(dtype, fmt):
    """one block: max-normal * 1.25 as amax (so the ceil rule has work to do), then 31 values spread over the binades below it, the last one
    below half the smallest quantum of the block's grid"""
    emax, mbits, emin, maxnorm = M.params(fmt)
    rng = np.random.default_rng(4)
    span = emax - (emin - mbits)                                             # binades from the format's top one down to its smallest quantum
    e = emax - (np.arange(31) * span / 30.0)
    v = (1.0 + 0.75 * rng.random(31)) * np.exp2(np.floor(e)) * rng.choice([-1.0, 1.0], 31)     # all below the amax
    v[30] = 0.3 * np.exp2(emin - mbits + 1)                                  # E(ceil) = 1: the smallest quantum is 2^(emin - mbits + 1)
    block = np.concatenate([[maxnorm * 1.25], v])
    return M.decode(M.encode(block, dtype), dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("fmt", FMTS)
def test_unbiased_under_ceil_where_nearest_is_not(fmt, dtype):
    """|mean(y) - x| <= 6 (hi - lo) / (2 sqrt N) + (hi - lo) 2^-16 at each of the 32 positions over N = 4096 tiles of one block: six sigma of a
    two-point variable (sigma <= (hi - lo) / 2) plus the stated bias of the 16-bit comparison.  Nearest rounding breaks the bound at the
    position below half a quantum (it rounds to zero every time): the bias this feature removes."""
    N = 4096
    x = unbiased_block(dtype, fmt)
    b = np.tile(M.encode(x, dtype), N)
    p = S.parts(b, dtype, fmt, "ceil", 0x5EED5EED5EED5EED, 3)
    y = M.decode(M.encode(p["y"], dtype), dtype).reshape(N, 32)
    lo, hi = p["lo"].reshape(N, 32)[0], p["hi"].reshape(N, 32)[0]
    bound = 6.0 * (hi - lo) / (2.0 * np.sqrt(N)) + (hi - lo) * 2.0 ** -16
    err = np.abs(y.mean(axis=0) - x)
    assert (err <= bound).all(), (np.flatnonzero(err > bound), err, bound)
    assert 0 < np.abs(x[31]) < 0.5 * (hi[31] - lo[31]) and lo[31] == 0                 # the position nearest rounding loses
    near = M.decode(R.quantize_bits(b, dtype, fmt, "ceil"), dtype).reshape(N, 32)
    nerr = np.abs(near.mean(axis=0) - x)
    assert near[:, 31].max() == 0 and nerr[31] == np.abs(x[31]) > bound[31]
