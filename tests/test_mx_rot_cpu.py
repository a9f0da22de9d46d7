"""The block-Hadamard rotation of the MX path, CPU tier (no GPU): the numpy reference against x @ H64 / 8 in float64, worked values, the
argument errors of the Python API, every validation code of the three new entry points (validation comes before any launch), the header /
EXPORTS agreement, and the accuracy claim on the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_reference import decode, quantize_values
from mx_rot_reference import RUN, export_rot_bits, hadamard64, quantize_rot_bits, rotate_bits, rotate_f32, rotate_values


def test_reference_equals_hadamard_product_on_integers():
    """|x| <= 256 integers: every partial sum is an integer below 2^24 and the final /8 is exact, so fp32 and float64 agree exactly"""
    rng = np.random.default_rng(0)
    x = rng.integers(-256, 257, (128, 256)).astype(np.float32)
    want = (x.astype(np.float64).reshape(-1, RUN) @ hadamard64() / 8).reshape(x.shape)
    got = rotate_f32(x)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_reference_is_its_own_inverse_on_integers():
    rng = np.random.default_rng(1)
    x = rng.integers(-256, 257, (64, 192)).astype(np.float32)
    assert np.array_equal(rotate_f32(rotate_f32(x)), x)
    h = hadamard64() / 8
    assert np.array_equal(h @ h, np.eye(RUN)) and np.array_equal(h, h.T)


def test_worked_values():
    e = np.zeros(64, np.float32)
    e[0] = 8.0
    assert rotate_f32(e).tolist() == [1.0] * 64                       # row 0 of H64 is all ones
    e = np.zeros(64, np.float32)
    e[1] = 8.0
    assert rotate_f32(e).tolist() == [1.0, -1.0] * 32                  # row 1 alternates
    e = np.zeros(64, np.float32)
    e[37] = -16.0                                                      # 37 = 0b100101
    assert rotate_f32(e).tolist() == [-2.0 * (-1) ** bin(37 & j).count("1") for j in range(64)]
    assert rotate_f32(np.ones(64, np.float32)).tolist() == [8.0] + [0.0] * 63
    r = rotate_f32(np.arange(64, dtype=np.float32))
    assert r[0] == 252.0 and [r[1], r[2], r[4], r[8], r[16], r[32]] == [-4.0, -8.0, -16.0, -32.0, -64.0, -128.0]
    assert np.count_nonzero(r) == 7
    # the outlier of a block is spread: one 64.0 among zeros becomes 64 values of 8.0, exactly representable in mxfp4 with E = 1
    x = np.zeros(64, np.float32)
    x[5] = 64.0
    q = decode(quantize_rot_bits(x.view(np.uint32), "fp32", "mxfp4"), "fp32")
    assert np.array_equal(np.abs(q), np.full(64, 8.0)) and np.array_equal(q, rotate_f32(x))


def test_overflowing_sum_and_non_finite_inputs_make_nan_blocks():
    big = np.full(64, 3e38, np.float32)
    r = rotate_f32(big)
    assert not np.isfinite(r[0])                                       # 3e38 + 3e38 overflows before the 0.125
    y = quantize_values(r.view(np.uint32), "fp32", "mxfp8_e4m3").reshape(2, 32)
    assert np.isnan(y[0]).all()
    codes, scales = export_rot_bits(big.view(np.uint32), "fp32", "mxfp8_e4m3")
    assert scales[0] == 0xFF
    for bad in (np.nan, np.inf, -np.inf):
        x = np.ones(128, np.float32)
        x[70] = bad
        y = decode(quantize_rot_bits(x.view(np.uint32), "fp32", "mxfp4"), "fp32")
        assert np.isfinite(y[:64]).all() and np.isnan(y[64:]).all()    # the run of the bad element only: both of its blocks
    z = decode(rotate_bits(np.zeros(64, np.uint16), "bf16"), "bf16")
    assert np.array_equal(z, np.zeros(64)) and not np.signbit(z).any()


def test_one_rounding_to_the_dtype():
    """the rotation-only form rounds the fp32 value once: 1 + 2^-9 is no bf16 value, the rotated sums are"""
    x = np.zeros(64, np.float32)
    x[0], x[1] = 8.0, 2.0 ** -6
    bits16 = (x.view(np.uint32) >> 16).astype(np.uint16)               # both exact in bf16
    r = rotate_values(bits16, "bf16")
    assert r[0] == np.float32(1.0 + 2.0 ** -9) and r[1] == np.float32(1.0 - 2.0 ** -9)
    got = decode(rotate_bits(bits16, "bf16"), "bf16")
    assert got[0] == 1.0 and got[1] == 1.0                             # RNE to 8 bits of precision


def _bf16_round(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_accuracy_claim_outlier_channels():
    """bf16 [512, 4096], one channel in 128 scaled x30: the rotated mxfp4 error is below 0.8 of the plain one (measured 0.65)"""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((512, 4096)) * np.where(np.arange(4096) % 128 == 5, 30, 1)[None, :]
    bits = _bf16_round(x)
    v = decode(bits, "bf16")
    plain = np.linalg.norm(quantize_values(bits, "bf16", "mxfp4").reshape(v.shape) - v) / np.linalg.norm(v)
    r = rotate_values(bits, "bf16")
    yr = quantize_values(r.view(np.uint32), "fp32", "mxfp4").reshape(v.shape)
    rot = np.linalg.norm(yr - r) / np.linalg.norm(r)
    back = np.linalg.norm(rotate_f32(yr.astype(np.float32)).astype(np.float64) - v) / np.linalg.norm(v)   # the same error seen in x's basis
    print(f"mxfp4 relative error: plain {plain:.4f}, rotated {rot:.4f} ({rot / plain:.3f}), back in x's basis {back:.4f}")
    assert rot < 0.8 * plain
    assert abs(back - rot) < 1e-3 * rot


# ---- Python API argument errors ---------------------------------------------------------------------------------------------------------

def test_ops_argument_errors():
    assert ops.MX_ROTATE == 64
    x = torch.zeros(4, 96)
    for call in (lambda: ops.mx_rotate(x), lambda: ops.mx_quantize(x, "mxfp4", rotate=True), lambda: ops.mx_export(x, "mxfp4", rotate=True),
                 lambda: llm_qat_amd.mx_quantize(x, "mxfp4", rotate=True), lambda: llm_qat_amd.block_rotate(x)):
        with pytest.raises(ValueError):
            call()                                                     # 96 is a multiple of 32, not of 64
    with pytest.raises(ValueError):
        ops.mx_quantize(torch.zeros(4, 128), "mxfp5", rotate=True)
    with pytest.raises(ValueError):
        ops.mx_export(torch.zeros(4, 128), "mxfp6_e2m3", rotate=True)  # FP6 export stays refused
    with pytest.raises(TypeError):
        llm_qat_amd.block_rotate([1.0] * 64)
    x = torch.zeros(4, 128)
    for allow in (False, True):                                        # CPU tensors raise, as on the rest of the MX path
        llm_qat_amd.allow_cpu_tensors(allow)
        try:
            for call in (lambda: ops.mx_rotate(x), lambda: ops.mx_quantize(x, "mxfp4", rotate=True),
                         lambda: ops.mx_export(x, "mxfp8_e4m3", rotate=True), lambda: llm_qat_amd.block_rotate(x),
                         lambda: llm_qat_amd.mx_quantize(x, "mxfp4", rotate=True)):
                with pytest.raises(RuntimeError):
                    call()
        finally:
            llm_qat_amd.allow_cpu_tensors(False)


def test_mx_export_rotated_flag_and_matmul_mismatch():
    e = torch.zeros(4, 64, dtype=torch.uint8)
    s = torch.zeros(4, 4, dtype=torch.uint8)
    plain = ops.MXExport(e, s, "mxfp4", (4, 128), torch.bfloat16)               # the five-argument constructor keeps working
    assert plain.rotated is False and "rotated" not in repr(plain)
    rot = ops.MXExport(e, s, "mxfp4", (4, 128), torch.bfloat16, True)
    assert rot.rotated is True and "rotated=True" in repr(rot)
    assert ops.MXExport(e, s, "mxfp4", (4, 128), torch.bfloat16, rotated=True).rotated is True
    assert torch.equal(rot.dequantize(), plain.dequantize())                    # dequantize() gives the values in the rotated basis
    for a, w in ((plain, rot), (rot, plain)):
        with pytest.raises(ValueError, match="rotat"):
            ops.mx_matmul(a, w)
    with pytest.raises(RuntimeError):                                           # matching flags pass the check and reach the CPU refusal
        ops.mx_matmul(rot, rot)


def test_quantize_linear_mx_rotate_argument_errors():
    m = QuantizeLinear(128, 32, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=True)
    assert m.mx_rotate is True and set(m.state_dict()) == {"weight"}
    assert QuantizeLinear(128, 32, weight_format="mxfp4", act_format="mxfp8_e4m3").mx_rotate is False
    with pytest.raises(ValueError):
        QuantizeLinear(128, 32, w_bits=4, a_bits=8, weight_format="mxfp4", mx_rotate=True)        # activations keep the integer quantizer
    with pytest.raises(ValueError):
        QuantizeLinear(128, 32, w_bits=4, a_bits=8, act_format="mxfp8_e4m3", mx_rotate=True)
    with pytest.raises(ValueError):
        QuantizeLinear(128, 32, w_bits=4, a_bits=8, mx_rotate=True)
    with pytest.raises(ValueError):
        QuantizeLinear(96, 32, weight_format="mxfp4", act_format="mxfp4", mx_rotate=True)         # 96 % 64
    assert QuantizeLinear(96, 32, weight_format="mxfp4", act_format="mxfp4").mx_rotate is False


def test_default_mx_rotate():
    import inspect
    assert list(inspect.signature(llm_qat_amd.default_mx_formats).parameters) == ["weight", "act"]
    assert llm_qat_amd.default_mx_rotate(True) is False
    try:
        assert QuantizeLinear(128, 32, weight_format="mxfp4", act_format="mxfp8_e4m3").mx_rotate is True
        assert QuantizeLinear(128, 32, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=False).mx_rotate is False
        assert QuantizeLinear(128, 32, w_bits=4, a_bits=8).mx_rotate is False                     # no formats: nothing to rotate
        assert QuantizeLinear(128, 32, weight_format="mxfp4").mx_rotate is False                  # one operand only: not rotated
        assert QuantizeLinear(96, 32, weight_format="mxfp4", act_format="mxfp4").mx_rotate is False
        prev = llm_qat_amd.default_mx_formats(weight="mxfp4", act="mxfp8_e4m3")
        try:
            assert prev == (None, None)
            m = QuantizeLinear(128, 32, bias=False, w_bits=4, a_bits=8)                            # unchanged model code
            assert (m.weight_format, m.act_format, m.mx_rotate) == ("mxfp4", "mxfp8_e4m3", True)
        finally:
            llm_qat_amd.default_mx_formats()
    finally:
        assert llm_qat_amd.default_mx_rotate(False) is True
    assert QuantizeLinear(128, 32, weight_format="mxfp4", act_format="mxfp8_e4m3").mx_rotate is False


def test_mx_linear_rotate_attribute():
    from llm_qat_amd import MXLinear, convert_to_mx_inference
    m = MXLinear(128, 32)
    assert m.rotate is False and "rotate" not in m.extra_repr()
    assert m.weight_export().rotated is False
    r = MXLinear(128, 32, rotate=True)
    assert r.rotate is True and "rotate=True" in r.extra_repr()
    assert r.weight_export().rotated is True
    assert set(r.state_dict()) == set(m.state_dict())
    q = QuantizeLinear(128, 32, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=True)
    with pytest.raises(RuntimeError):                                  # eligible; the export then refuses the CPU weight
        MXLinear.from_quantize_linear(q)
    with pytest.raises(RuntimeError):
        convert_to_mx_inference(torch.nn.Sequential(q))


# ---- C ABI: header, EXPORTS and validation codes (no launch) ------------------------------------------------------------------------------

NEW = {"fq_mx_fwd_rot": "ppqqiip", "fq_mx_export_rot": "pppqqiip", "fq_block_rotate": "ppqqip"}


def test_header_declares_the_new_entry_points_and_exports_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "llmqat_fakequant.h")).read()
    assert re.search(r"^#define FQ_ABI_VERSION 7\b", hdr, re.M)
    L = _lib.lib()
    for name, kinds in NEW.items():
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, re.M | re.S)
        assert m, f"{name} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        got = "".join("p" if "*" in a else "q" if a.startswith("int64_t") else "i" for a in args)
        assert got == kinds
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert "".join("p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64 else "i" for t in fn.argtypes) == kinds


def test_abi_validation_codes_of_the_rotated_entry_points():
    L = _lib.lib()
    assert L.fq_version() == 7
    fake = 1 << 20        # a 16-byte-aligned non-NULL address: never dereferenced, validation fails first
    BF, F16, F32, F64 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32, _lib.DTYPE_F64
    fwd, exp, rot = L.fq_mx_fwd_rot, L.fq_mx_export_rot, L.fq_block_rotate
    assert fwd(fake, fake + 4096, 4, 64, 0, F64, None) == -1
    assert fwd(fake, fake + 4096, 4, 64, 0, 9, None) == -1
    assert fwd(fake, fake + 4096, 4, 64, 5, BF, None) == -7
    assert fwd(fake, fake + 4096, 4, 64, -1, BF, None) == -7
    assert fwd(fake, fake, 4, 64, 0, BF, None) == -7                 # y == x
    assert fwd(fake, fake + 4096, 4, 96, 0, BF, None) == -3          # a multiple of 32, not of 64
    assert fwd(fake, fake + 4096, 4, 32, 1, F32, None) == -3
    assert fwd(fake, fake + 4096, -1, 64, 0, BF, None) == -3
    assert fwd(None, fake, 4, 64, 0, BF, None) == -4
    assert fwd(fake, None, 4, 64, 0, BF, None) == -4
    assert fwd(fake + 2, fake + 4096, 4, 64, 0, BF, None) == -8
    assert fwd(fake, fake + 4096 + 8, 4, 64, 0, F32, None) == -8
    assert fwd(None, None, 0, 64, 0, BF, None) == 0                  # empty: no launch
    assert fwd(None, None, 5, 0, 2, F16, None) == 0
    assert exp(fake, fake + 4096, fake + 8192, 4, 64, 1, BF, None) == -7    # FP6 export
    assert exp(fake, fake + 4096, fake + 8192, 4, 64, 2, F32, None) == -7
    assert exp(fake, fake + 4096, fake + 8192, 4, 64, 7, F32, None) == -7
    assert exp(fake, fake + 4096, fake + 8192, 4, 64, 0, F64, None) == -1
    assert exp(fake, fake + 4096, fake + 8192, 4, 96, 3, F16, None) == -3
    assert exp(fake, None, fake + 8192, 4, 64, 3, F16, None) == -4
    assert exp(fake, fake + 4096, None, 4, 64, 3, F16, None) == -4
    assert exp(None, fake + 4096, fake + 8192, 4, 64, 3, F16, None) == -4
    assert exp(fake, fake + 4096, fake + 8200, 4, 64, 3, F16, None) == -8
    assert exp(fake, fake + 4100, fake + 8192, 4, 64, 0, F16, None) == -8
    assert exp(None, None, None, 7, 0, 4, F32, None) == 0
    assert rot(fake, fake + 4096, 4, 64, F64, None) == -1
    assert rot(fake, fake + 4096, 4, 64, -1, None) == -1
    assert rot(fake, fake, 4, 64, BF, None) == -7                    # y == x
    assert rot(fake, fake + 4096, 4, 32, BF, None) == -3
    assert rot(fake, fake + 4096, 4, 160, F32, None) == -3
    assert rot(fake, fake + 4096, 4, -64, F32, None) == -3
    assert rot(None, fake, 4, 64, BF, None) == -4
    assert rot(fake, None, 4, 64, BF, None) == -4
    assert rot(fake + 4, fake + 4096, 4, 64, F32, None) == -8
    assert rot(None, None, 0, 64, F16, None) == 0
