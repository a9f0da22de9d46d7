"""CPU tier of the MX dequantize kernel and MXLinear's dequantized route: the fqi_ header and its binding, every
refusal of fqi_mx_dequant in the order the header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers
below are never dereferenced), the Python argument checks, the fake implementation of the compiled op, and a sensitivity check of the
exhaustive case set the GPU tier runs, done on the reference alone."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

from llm_qat_amd import _lib, compiled, mx_inference, ops
from llm_qat_amd.mx_inference import MXLinear, convert_to_mx_inference
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_dequant_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, S = 0x1000, 0x2000, 0x3001           # A, B 16-byte aligned; S (the scales) need not be; never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
FP4, E2M3, E3M2, E4M3, E5M2 = range(5)
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 11008, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]


def call(elems, scales, y, rows, cols, fmt, dtype):
    L = _lib.lib()
    rc = L.fqi_mx_dequant(elems, scales, y, rows, cols, fmt, dtype, None)
    return rc, L.fq_last_error().decode()


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_infer_header_names_equal_infer_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_infer.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqi_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.INFER_EXPORTS) == {"fqi_mx_dequant"}
    assert not re.findall(r"\bfq[ts]?_[a-z0-9_]+\s*\(", src)       # nothing of the three other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert not set(_lib.INFER_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS))
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.fqi_mx_dequant.argtypes == [vp, vp, vp, i64, i64, i32, i32, vp] and L.fqi_mx_dequant.restype is i32


def test_the_build_lists_the_new_unit_and_headers():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_mx_dequant.hip", "fq_mx_dequant.h", "llmqat_fakequant_infer.h"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

REFUSALS = [
    # (elems, scales, y, rows, cols, fmt, dtype), code, part of the message
    ((None, None, None, -1, -1, 9, 9), DTYPE, "unknown dtype"),
    ((None, None, None, -1, -1, 9, -1), DTYPE, "unknown dtype"),
    ((None, None, None, -1, -1, 9, F64), DTYPE, "float64"),
    ((None, None, None, -1, -1, 5, BF16), ARG, "unknown MX format"),
    ((None, None, None, -1, -1, -1, F32), ARG, "unknown MX format"),
    ((None, None, None, -1, -1, E2M3, BF16), ARG, "FP6 formats have no export packing"),
    ((None, None, None, -1, 33, E3M2, F16), ARG, "FP6 formats have no export packing"),
    ((None, None, None, -3, 32, FP4, BF16), SHAPE, "negative shape"),
    ((None, None, None, 3, -32, E4M3, BF16), SHAPE, "negative shape"),
    ((None, None, None, 3, 33, E4M3, BF16), SHAPE, "cols=33 is not a multiple of the 32"),
    ((None, None, None, 0, 16, E5M2, F32), SHAPE, "not a multiple"),                   # cols % 32 comes before the empty shape
    ((None, None, None, 2 ** 62, 2 ** 40, FP4, BF16), SHAPE, "overflows"),
    ((None, S, B, 3, 32, FP4, BF16), NULL, "NULL"),
    ((A, None, B, 3, 32, FP4, BF16), NULL, "NULL"),
    ((A, S, None, 3, 32, FP4, BF16), NULL, "NULL"),
    ((None, None, None, 3, 32, E4M3, F32), NULL, "NULL"),
    ((A + 2, S, B, 3, 32, FP4, BF16), UNSUPPORTED, "16-byte aligned"),
    ((A, S, B + 8, 3, 32, E5M2, F32), UNSUPPORTED, "16-byte aligned"),
    ((A + 1, S, B + 4, 2 ** 45, 2 ** 14, E4M3, F16), UNSUPPORTED, "16-byte aligned"),  # the alignment comes before the grid
    ((A, S, B, 2 ** 45, 2 ** 14, FP4, BF16), UNSUPPORTED, "exceed one launch's grid"),
]


@pytest.mark.parametrize("args, code, text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_in_the_stated_order(args, code, text):
    rc, msg = call(*args)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_the_fp6_refusal_is_the_export_entry_points():
    L = _lib.lib()
    for fmt in (E2M3, E3M2):
        rc = L.fq_mx_export(None, None, None, -1, -1, fmt, BF16, None)
        want = (rc, L.fq_last_error().decode())
        assert call(None, None, None, -1, -1, fmt, BF16) == want and want[0] == ARG


def test_every_served_format_and_dtype_passes_the_first_checks():
    for fmt in (FP4, E4M3, E5M2):
        for dtype in (F32, BF16, F16):
            assert call(None, None, None, 3, 32, fmt, dtype)[0] == NULL      # all the checks before the pointers passed


def test_empty_shapes_return_zero_without_a_launch():
    for rows, cols in ((0, 32), (3, 0), (0, 0), (0, 64), (64, 0)):
        rc, msg = call(None, None, None, rows, cols, E4M3, BF16)
        assert rc == 0 and msg == "", (rows, cols, rc, msg)


def test_fuzz_never_reaches_a_launch():
    rng = random.Random(21)
    L = _lib.lib()
    seen = set()
    for _ in range(400):
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        fmt, dtype = (max(-(2 ** 31), min(2 ** 31 - 1, rng.choice(INTS))) for _ in range(2))
        rc = L.fqi_mx_dequant(None, None, None, rows, cols, fmt, dtype, None)
        assert rc in (0, DTYPE, ARG, SHAPE, NULL), (rc, rows, cols, fmt, dtype)
        assert rc != 0 or rows == 0 or cols == 0
        assert rc != 0 or L.fq_last_error() == b""
        seen.add(rc)
    assert {DTYPE, ARG} <= seen
    for _ in range(400):       # the same hostile sizes behind valid codes, so that the shape checks are the ones that answer
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        rc = L.fqi_mx_dequant(None, None, None, rows, cols, rng.choice((FP4, E4M3, E5M2)), rng.randrange(3), None)
        assert rc in (0, SHAPE, NULL), (rc, rows, cols)
        assert (rc == 0) == (rows >= 0 and cols >= 0 and cols % 32 == 0 and (rows == 0 or cols == 0)), (rc, rows, cols)


# ---- Python argument checks (all before any launch; the device check is the last of them, so CPU tensors reach the others) --------------------

def _export(fmt="mxfp4", shape=(4, 64), dtype=torch.bfloat16):
    return ops.MXExport(torch.zeros(shape[0], shape[1] // 2 if fmt == "mxfp4" else shape[1], dtype=torch.uint8),
                        torch.zeros(shape[0], shape[1] // 32, dtype=torch.uint8), fmt, shape, dtype)


def test_python_argument_errors_of_mx_dequantize():
    e = _export()
    with pytest.raises(TypeError, match="MXExport"):
        ops.mx_dequantize(torch.zeros(4, 64))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mx_dequantize(e)                                          # the arguments are fine: what is left is the device
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mx_dequantize(e, dtype=torch.float32)
    with pytest.raises(ValueError, match="not served"):
        ops.mx_dequantize(e, dtype=torch.float64)
    with pytest.raises(ValueError, match="not served"):
        ops.mx_dequantize(_export(dtype=torch.float64))
    with pytest.raises(ValueError, match="not served"):
        ops.mx_dequantize(e, dtype=torch.int8)
    for fmt in ("mxfp6_e2m3", "mxfp6_e3m2"):
        with pytest.raises(ValueError, match="FP6 formats have no export packing"):
            ops.mx_dequantize_tensors(e.elements, e.scales, fmt, e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="unknown MX format"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp5", e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp4", (4, 48), torch.bfloat16)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp4", (), torch.bfloat16)
    with pytest.raises(TypeError, match="uint8"):
        ops.mx_dequantize_tensors(e.elements.float(), e.scales, "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(TypeError, match="uint8"):
        ops.mx_dequantize_tensors(e.elements, e.scales.to(torch.int8), "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(TypeError, match="uint8"):
        ops.mx_dequantize_tensors(e.elements, None, "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="elements holds 128 bytes"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp8_e4m3", e.shape, torch.bfloat16)      # fp4's byte count under an fp8 format
    with pytest.raises(ValueError, match="elements holds 127 bytes"):
        ops.mx_dequantize_tensors(e.elements.reshape(-1)[1:], e.scales, "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="scales holds 7 bytes"):
        ops.mx_dequantize_tensors(e.elements, e.scales.reshape(-1)[1:], "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="elements holds 128 bytes"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp4", (8, 64), torch.bfloat16)
    assert list(inspect.signature(ops.mx_dequantize).parameters) == ["e", "dtype"]
    assert inspect.signature(ops.mx_dequantize).parameters["dtype"].default is None
    assert list(inspect.signature(ops.mx_dequantize_tensors).parameters) == ["elements", "scales", "fmt", "shape", "dtype"]
    assert ops.mx_counts["mx_dequant_launch"] == 0


def test_check_mx_dequant_counts_the_elements():
    assert ops.check_mx_dequant("mxfp4", (4, 64), torch.bfloat16) == 256
    assert ops.check_mx_dequant("mxfp8_e5m2", (2, 3, 32), torch.float32) == 192
    assert ops.check_mx_dequant("mxfp8_e4m3", (0, 32), torch.float16) == 0


def test_mx_linear_dequant_above_argument():
    for bad in (-1, True, False, "32", 1.0, 2.5, (1,)):
        with pytest.raises(ValueError, match="dequant_above"):
            MXLinear(128, 96, dequant_above=bad)
    with pytest.raises(ValueError, match="dequant_above"):
        convert_to_mx_inference(torch.nn.Sequential(), dequant_above=-2)
    plain, routed, zero = MXLinear(128, 96), MXLinear(128, 96, dequant_above=32), MXLinear(128, 96, bias=True, dequant_above=0)
    assert plain.dequant_above is None and routed.dequant_above == 32 and zero.dequant_above == 0
    assert "dequant_above" not in plain.extra_repr() and "dequant_above=32" in routed.extra_repr() and "dequant_above=0" in zero.extra_repr()
    assert set(plain.state_dict()) == set(routed.state_dict()) == {"weight_elements", "weight_scales"}
    assert set(zero.state_dict()) == {"weight_elements", "weight_scales", "bias"}
    routed.load_state_dict(plain.state_dict())
    plain.load_state_dict(routed.state_dict())
    for f in (MXLinear.__init__, MXLinear.from_quantize_linear, convert_to_mx_inference):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "dequant_above" and p["dequant_above"].default is None
    d = mx_inference.DEQUANT_ABOVE_DEFAULT
    assert d is None or (isinstance(d, int) and not isinstance(d, bool) and d >= 0)
    assert "DEQUANT_ABOVE_DEFAULT" in MXLinear.__doc__ and "transient" in MXLinear.__doc__
    with pytest.raises(RuntimeError, match="no CPU"):
        zero(torch.zeros(2, 128))
    layer = QuantizeLinear(128, 96, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3")
    with pytest.raises(ValueError, match="dequant_above"):
        MXLinear.from_quantize_linear(layer, dequant_above="0")


# ---- the compiled op's fake implementation ----------------------------------------------------------------------------------------------------

def test_fake_op_shape_and_dtype_on_meta_tensors():
    assert str(compiled.mx_dequant_op._opoverload._schema) == \
        "llmqat_amd::mx_dequant(Tensor elements, Tensor scales, str fmt, SymInt[] shape, ScalarType dtype) -> Tensor"
    for fmt, per in (("mxfp4", 2), ("mxfp8_e4m3", 1), ("mxfp8_e5m2", 1)):
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            for shape in ((96, 256), (2, 3, 64), (0, 32)):
                n = int(np.prod(shape))
                e = torch.empty(n // per, dtype=torch.uint8, device="meta")
                s = torch.empty(n // 32, dtype=torch.uint8, device="meta")
                y = torch.ops.llmqat_amd.mx_dequant(e, s, fmt, list(shape), dtype)
                assert y.device.type == "meta" and tuple(y.shape) == shape and y.dtype is dtype and y.is_contiguous()
    e, s = torch.empty(64, dtype=torch.uint8, device="meta"), torch.empty(4, dtype=torch.uint8, device="meta")
    with pytest.raises(ValueError, match="FP6"):
        torch.ops.llmqat_amd.mx_dequant(e, s, "mxfp6_e2m3", [4, 32], torch.bfloat16)
    with pytest.raises(ValueError, match="not served"):
        torch.ops.llmqat_amd.mx_dequant(e, s, "mxfp4", [4, 32], torch.float64)
    with pytest.raises(ValueError, match="multiple of 32"):
        torch.ops.llmqat_amd.mx_dequant(e, s, "mxfp4", [4, 40], torch.bfloat16)


# ---- the exhaustive case set, on the reference alone --------------------------------------------------------------------------------------------

def _count(b, dtype):
    """(NaN, Inf, subnormal) outputs among the bit patterns b"""
    ebits, mbits = {"bf16": (0x7F80, 0x7F), "fp16": (0x7C00, 0x3FF), "fp32": (0x7F800000, 0x7FFFFF)}[dtype]
    e, m = b & ebits, b & mbits
    return int(((e == ebits) & (m != 0)).sum()), int(((e == ebits) & (m == 0)).sum()), int(((e == 0) & (m != 0)).sum())


def test_the_exhaustive_set_holds_every_code_under_every_scale_and_the_hard_results():
    for fmt in C.FMTS:
        elements, scales, shape = C.exhaustive(fmt)
        assert elements.dtype == scales.dtype == torch.uint8 and shape == (256, 32 if fmt == "mxfp4" else 256)
        assert scales.shape == (256, shape[1] // 32) and (scales == torch.arange(256).reshape(-1, 1)).all()      # row s: byte s, every block
        codes = C.codes_of(fmt)
        assert sorted(set(codes.tolist())) == list(range(16 if fmt == "mxfp4" else 256))
        if fmt == "mxfp4":
            lo, hi = (elements & 0xF).numpy(), (elements >> 4).numpy()
            assert all(set(lo[r].tolist()) == set(hi[r].tolist()) == set(range(16)) for r in range(256))       # every code in both nibbles
    # the figures the kernel's open questions hang on (hardware converts, flushing): the set does contain NaN, +-Inf, dtype-subnormal results
    got = {}
    for dtype in C.DTYPES:
        elements, scales, shape = C.exhaustive("mxfp8_e4m3")
        got[dtype] = _count(C.bits(C.reference(elements, scales, "mxfp8_e4m3", shape, dtype), dtype), dtype)
    assert got["bf16"] == (766, 560, 554), got
    assert got["fp16"][1] == 28342, got
    assert got["fp32"][2] > 0, got                         # fp32 subnormals: what a flushing kernel would lose
    for fmt in C.FMTS:
        for dtype in C.DTYPES:
            elements, scales, shape = C.exhaustive(fmt)
            b = C.bits(C.reference(elements, scales, fmt, shape, dtype), dtype)
            nan, inf, sub = _count(b, dtype)
            assert nan >= shape[1] and sub > 0, (fmt, dtype, nan, inf, sub)
            assert (b == (0x80000000 if dtype == "fp32" else 0x8000)).any()                # -0 is among the results
            # roundings to zero of a non-zero code: in fp16 for every format; in bf16 (smallest subnormal 2^-133) for the FP8 formats,
            # whose smallest codes times 2^-127 lie below it (FP4's 0.5 * 2^-127 does not); never in fp32, where every product is exact
            nz = C.finite_nonzero(fmt)[C.codes_of(fmt)]
            zero = (b & (0x7FFFFFFF if dtype == "fp32" else 0x7FFF)) == 0
            assert zero[:, nz].any() == (dtype == "fp16" or (dtype == "bf16" and fmt != "mxfp4")), (fmt, dtype)


def test_a_scale_off_by_one_changes_every_row():
    """fp32 and bf16 share fp32's exponent range, where two neighbouring scales never give the same row (the smallest product, 2^-143, is
    an fp32 value; only the largest e5m2 codes overflow under the largest scales, never a whole row).  fp16 rows under scales that push
    every non-zero code to Inf or to 0 cannot tell two scales apart, so there the check covers the rows that hold a finite non-zero
    result, whose neighbour must differ."""
    for fmt in C.FMTS:
        elements, scales, shape = C.exhaustive(fmt)
        for dtype in C.DTYPES:
            right = C.bits(C.reference(elements, scales, fmt, shape, dtype), dtype)
            for off in (1, 255):                                                            # one up, one down (mod 256)
                wrong = C.bits(C.reference(elements, scales + off, fmt, shape, dtype), dtype)
                same = np.array([_row_bits_equal(right[r], wrong[r], dtype) for r in range(256)])
                if dtype == "fp16":
                    emask, full = 0x7C00, 0x7FFF
                    live = np.array([(((right[r] & emask) != emask) & ((right[r] & full) != 0)).any() for r in range(256)])
                    assert live.sum() > 30 and not same[live].any(), (fmt, dtype, off, np.flatnonzero(same & live))
                else:
                    assert not same.any(), (fmt, dtype, off, np.flatnonzero(same))


def test_an_element_table_off_by_one_step_changes_every_finite_nonzero_code():
    for fmt in C.FMTS:
        elements, scales, shape = C.exhaustive(fmt)
        table = C.next_code(fmt)
        ok = C.finite_nonzero(fmt)
        assert (table[ok] != np.arange(len(table))[ok]).all() and (table[~ok] == np.arange(len(table))[~ok]).all()
        col_ok = ok[C.codes_of(fmt)]
        for dtype in C.DTYPES:
            right = C.bits(C.reference(elements, scales, fmt, shape, dtype), dtype)
            wrong = C.bits(C.reference(C.remap(elements, fmt, table), scales, fmt, shape, dtype), dtype)
            differs = right != wrong
            assert differs[127][col_ok].all(), (fmt, dtype)                   # under scale 1 every such code's value is a dtype value
            assert differs[:, col_ok].any(0).all() and not differs[:, ~col_ok].any(), (fmt, dtype)


def _row_bits_equal(a, b, dtype):
    from conftest import bits_equal
    return bits_equal(a.view(np.float32) if dtype == "fp32" else a, b.view(np.float32) if dtype == "fp32" else b, dtype)
