"""OCP MX block-scaled fake quantization, CPU tier: the worked values of the format through the numpy reference, the reference against
torch's own float8 casts, the argument errors of the Python API, the C ABI's validation codes (no launch) and MXExport.dequantize() on CPU
tensors built from reference codes."""
import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_reference import FORMATS, decode, export_bits, pack_fp4, params, quantize_bits, quantize_values, shared_exp


def f32_block(first, rest=()):
    v = np.zeros(32, dtype=np.float32)
    v[0] = first
    v[1:1 + len(rest)] = rest
    return v.view(np.uint32)


def ref_values(block_bits, fmt, dtype="fp32"):
    return decode(quantize_bits(block_bits, dtype, fmt), dtype)


def test_worked_values_mxfp4_amax_5():
    b = f32_block(5.0, [2.5, 0.75, 0.25, 0.3, -0.2])
    assert shared_exp(np.array([5.0]), "mxfp4")[0] == 0
    y = ref_values(b, "mxfp4")
    assert list(y[:6]) == [4.0, 2.0, 1.0, 0.0, 0.5, -0.0]
    assert not np.signbit(y[3]) and np.signbit(y[5])     # 0.25 -> +0, -0.2 -> -0


def test_worked_values_saturation_band_and_small_amax():
    y = ref_values(f32_block(7.5), "mxfp4")
    assert shared_exp(np.array([7.5]), "mxfp4")[0] == 0 and y[0] == 6.0
    y = ref_values(f32_block(np.float32(0.1)), "mxfp4")
    assert shared_exp(np.array([np.float32(0.1)], dtype=np.float64), "mxfp4")[0] == -6 and y[0] == 0.09375


def test_worked_values_mxfp8_e4m3():
    assert shared_exp(np.array([1000.0]), "mxfp8_e4m3")[0] == 1
    assert ref_values(f32_block(1000.0), "mxfp8_e4m3")[0] == 896.0   # t = 500 -> 512 -> saturates to 448


def test_format_parameters():
    assert {f: params(f) for f in FORMATS} == {"mxfp4": (2, 1, 0, 6.0), "mxfp6_e2m3": (2, 3, 0, 7.5), "mxfp6_e3m2": (4, 2, -2, 28.0),
                                              "mxfp8_e4m3": (8, 3, -6, 448.0), "mxfp8_e5m2": (15, 2, -14, 57344.0)}
    assert set(ops.MX_FORMATS) == set(FORMATS)


def test_non_finite_block_is_nan_with_nan_scale():
    for bad in (np.nan, np.inf, -np.inf):
        b = f32_block(1.0, [bad, 2.0])
        assert np.isnan(quantize_values(b, "fp32", "mxfp4")).all()
        codes, scales = export_bits(b, "fp32", "mxfp8_e4m3")
        assert scales[0] == 0xFF and (codes == 0).all()


def test_zero_and_subnormal_amax():
    assert shared_exp(np.array([0.0]), "mxfp4")[0] == -127
    assert shared_exp(np.array([2.0 ** -140]), "mxfp4")[0] == -127       # clamped
    assert shared_exp(np.array([2.0 ** -133]), "mxfp8_e5m2")[0] == -127
    assert shared_exp(np.array([3e38]), "mxfp4")[0] == 125
    b = (np.zeros(32, np.uint16))
    b[5] = 0x8000                                                           # -0 in bf16
    y = quantize_bits(b, "bf16", "mxfp4")
    assert y[5] == 0x8000 and (np.delete(y, 5) == 0).all()


@pytest.mark.parametrize("fmt,tdt", [("mxfp8_e4m3", torch.float8_e4m3fn), ("mxfp8_e5m2", torch.float8_e5m2)])
def test_fp8_elements_match_torch_casts_within_range(fmt, tdt):
    """q of the reference == torch's float8 cast of t, for |t| <= max-normal (torch's e4m3fn cast does not saturate: 500 -> NaN)"""
    emax, mbits, emin, maxnorm = params(fmt)
    rng = np.random.default_rng(1)
    for amax_exp in (-20, -3, 0, 5, 40):
        v = (rng.standard_normal((64, 32)) * 2.0 ** amax_exp).astype(np.float32)
        v[:, 3] = 0.0
        v[:, 4] = -v[:, 5] / 2 ** 12     # deep subnormal territory of the element grid
        E = shared_exp(np.abs(v.astype(np.float64)).max(1), fmt)
        t = v.astype(np.float64) * np.exp2(-E.astype(np.float64))[:, None]
        q = decode(quantize_bits(v.view(np.uint32), "fp32", fmt), "fp32") / np.exp2(E.astype(np.float64))[:, None]
        inr = np.abs(t) <= maxnorm
        tq = torch.from_numpy(t.astype(np.float32)).to(tdt).float().double().numpy()
        assert inr.mean() > 0.9
        assert np.array_equal(q[inr], tq[inr])
        assert np.array_equal(np.signbit(q[inr]), np.signbit(tq[inr]))


def test_export_codes_decode_to_the_reference_values():
    rng = np.random.default_rng(2)
    v = (rng.standard_normal(32 * 16) * 3).astype(np.float32)
    for fmt, tdt in (("mxfp8_e4m3", torch.float8_e4m3fn), ("mxfp8_e5m2", torch.float8_e5m2)):
        codes, scales = export_bits(v.view(np.uint32), "fp32", fmt)
        q = torch.from_numpy(codes).view(tdt).float().double().numpy().reshape(-1, 32)
        s = torch.from_numpy(scales).view(torch.float8_e8m0fnu).float().double().numpy()
        assert np.array_equal((q * s[:, None]).reshape(-1), quantize_values(v.view(np.uint32), "fp32", fmt))


# ---- the Python API's argument errors -----------------------------------------------------------------------------------------------------

def test_check_mx_errors():
    assert ops.check_mx((4, 64), "mxfp4") == _lib.MX_FP4_E2M1
    with pytest.raises(ValueError):
        ops.check_mx((4, 64), "mxfp3")
    with pytest.raises(ValueError):
        ops.check_mx((4, 48), "mxfp8_e4m3")
    with pytest.raises(ValueError):
        ops.check_mx((4, 64), None)


def test_ops_and_public_api_errors_on_cpu():
    x = torch.randn(4, 64)
    with pytest.raises(ValueError):
        ops.mx_quantize(torch.randn(4, 40), "mxfp4")
    with pytest.raises(ValueError):
        llm_qat_amd.mx_quantize(x, "nvfp4")
    with pytest.raises(ValueError):
        ops.mx_export(x, "mxfp6_e2m3")          # FP6: no packing
    for allow in (False, True):                  # CPU tensors raise, with or without allow_cpu_tensors
        llm_qat_amd.allow_cpu_tensors(allow)
        try:
            with pytest.raises(RuntimeError):
                ops.mx_quantize(x, "mxfp4")
            with pytest.raises(RuntimeError):
                llm_qat_amd.mx_quantize(x, "mxfp4")
            with pytest.raises(RuntimeError):
                ops.mx_export(x, "mxfp8_e5m2")
        finally:
            llm_qat_amd.allow_cpu_tensors(False)


def test_quantize_linear_argument_errors():
    with pytest.raises(ValueError):
        QuantizeLinear(64, 32, w_bits=4, weight_format="mxfp4", weight_group_size=32)
    with pytest.raises(ValueError):
        QuantizeLinear(64, 32, w_bits=4, weight_format="mxfp4", weight_layerwise=True)
    with pytest.raises(ValueError):
        QuantizeLinear(64, 32, a_bits=8, act_format="mxfp8_e4m3", act_group_size=32)
    with pytest.raises(ValueError):
        QuantizeLinear(64, 32, a_bits=8, act_format="mxfp8_e4m3", act_layerwise=True)
    with pytest.raises(ValueError):
        QuantizeLinear(64, 32, weight_format="mxfp5")
    with pytest.raises(ValueError):
        QuantizeLinear(48, 32, weight_format="mxfp4")          # in_features not a multiple of 32
    m = QuantizeLinear(64, 32, weight_format="mxfp6_e3m2")
    with pytest.raises(ValueError):
        m.export_weight()
    assert set(m.state_dict()) == {"weight"}


def test_default_mx_formats():
    with pytest.raises(ValueError):
        llm_qat_amd.default_mx_formats(weight="int4")
    with pytest.raises(ValueError):
        llm_qat_amd.default_mx_formats(act="mxfp4x")
    prev = llm_qat_amd.default_mx_formats(weight="mxfp4", act="mxfp8_e4m3")
    try:
        assert prev == (None, None)
        m = QuantizeLinear(64, 32, w_bits=4, a_bits=8)
        assert (m.weight_format, m.act_format) == ("mxfp4", "mxfp8_e4m3")
        m = QuantizeLinear(64, 32)                              # operands the layer does not quantize keep no format
        assert (m.weight_format, m.act_format) == (None, None)
        m = QuantizeLinear(64, 32, w_bits=4, a_bits=8, weight_layerwise=True, act_group_size=32)
        assert (m.weight_format, m.act_format, m.act_group_size) == (None, None, 32)
        m = QuantizeLinear(64, 32, act_format="mxfp8_e5m2")     # an explicit argument always applies
        assert (m.weight_format, m.act_format) == (None, "mxfp8_e5m2")
    finally:
        llm_qat_amd.default_mx_formats()
    assert QuantizeLinear(64, 32, w_bits=4, a_bits=8).weight_format is None


# ---- C ABI validation (no launch: every call returns before any HIP call) ------------------------------------------------------------

def test_abi_validation_codes():
    L = _lib.lib()
    assert L.fq_version() == 7
    fake = 1 << 20        # a 16-byte-aligned non-NULL address: never dereferenced, validation fails first
    assert L.fq_mx_fwd(fake, fake + 4096, 4, 64, 0, _lib.DTYPE_F64, None) == -1
    assert L.fq_mx_fwd(fake, fake + 4096, 4, 64, 0, 9, None) == -1
    assert L.fq_mx_fwd(fake, fake + 4096, 4, 64, 5, _lib.DTYPE_BF16, None) == -7
    assert L.fq_mx_fwd(fake, fake, 4, 64, 0, _lib.DTYPE_BF16, None) == -7           # y == x
    assert L.fq_mx_fwd(fake, fake + 4096, 4, 48, 0, _lib.DTYPE_BF16, None) == -3
    assert L.fq_mx_fwd(fake, fake + 4096, -1, 64, 0, _lib.DTYPE_BF16, None) == -3
    assert L.fq_mx_fwd(None, fake, 4, 64, 0, _lib.DTYPE_BF16, None) == -4
    assert L.fq_mx_fwd(fake + 2, fake + 4096, 4, 64, 0, _lib.DTYPE_BF16, None) == -8
    assert L.fq_mx_fwd(None, None, 0, 64, 0, _lib.DTYPE_BF16, None) == 0            # empty: no launch
    assert L.fq_mx_export(fake, fake + 4096, fake + 8192, 4, 64, 1, _lib.DTYPE_BF16, None) == -7   # FP6 export
    assert L.fq_mx_export(fake, fake + 4096, fake + 8192, 4, 64, 2, _lib.DTYPE_F32, None) == -7
    assert L.fq_mx_export(fake, fake + 4096, fake + 8192, 4, 64, 0, _lib.DTYPE_F64, None) == -1
    assert L.fq_mx_export(fake, fake + 4096, fake + 8192, 4, 40, 3, _lib.DTYPE_F16, None) == -3
    assert L.fq_mx_export(fake, None, fake + 8192, 4, 64, 3, _lib.DTYPE_F16, None) == -4
    assert L.fq_mx_export(fake, fake + 4096, fake + 8200, 4, 64, 3, _lib.DTYPE_F16, None) == -8
    assert L.fq_mx_export(None, None, None, 7, 0, 4, _lib.DTYPE_F32, None) == 0


# ---- MXExport.dequantize() on CPU tensors built from reference codes ----------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_dequantize_of_reference_codes(fmt, dtype):
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]
    x = (torch.randn(6, 128, generator=torch.Generator().manual_seed(4)) * torch.tensor(2.0) ** torch.randint(-12, 12, (6, 1))).to(tdt)
    x[0, 5] = -0.0
    x[1, :32] = 0.0
    x[1, 33] = float("nan")
    x[2, 70] = float("-inf")
    x[3, 100] = -x[3, 100].abs() / 2 ** 10
    bits = x.view(torch.int16 if dtype != "fp32" else torch.int32).numpy().view(np.uint16 if dtype != "fp32" else np.uint32).reshape(-1)
    codes, scales = export_bits(bits, dtype, fmt)
    elems = pack_fp4(codes) if fmt == "mxfp4" else codes
    e = ops.MXExport(torch.from_numpy(elems.reshape(6, -1)), torch.from_numpy(scales.reshape(6, -1)), fmt, (6, 128), tdt)
    got = e.dequantize()
    assert got.dtype is tdt and got.shape == (6, 128)
    want = quantize_bits(bits, dtype, fmt)
    gb = got.view(torch.int16 if dtype != "fp32" else torch.int32).numpy().view(want.dtype).reshape(-1)
    nan = np.isnan(decode(want, dtype))
    assert np.array_equal(np.isnan(decode(gb, dtype)), nan)
    assert np.array_equal(gb[~nan], want[~nan])     # bit for bit: signed zeros included
    assert nan.sum() == 64
