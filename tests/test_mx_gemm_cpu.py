"""MX block-scaled GEMM, CPU tier (no GPU): argument errors of ops.mx_matmul, every fq_mx_gemm validation code (validation comes before
any launch), the header / EXPORTS agreement, MXLinear eligibility and its state_dict, and the float64 reference on worked values."""
import os
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import MXLinear, _lib, convert_to_mx_inference, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_gemm_reference import codes_of_values, export_from_codes, grid_operand, prove_exact, ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _export(rows, K, fmt="mxfp4"):
    return export_from_codes(np.zeros((rows, K), np.uint8), np.full((rows, K // 32), 127, np.uint8), fmt)


def test_mx_matmul_argument_errors():
    a, w = _export(4, 256), _export(8, 256)
    with pytest.raises(TypeError):
        ops.mx_matmul(a.elements, w)
    with pytest.raises(ValueError, match="K=256 but w has K=128"):
        ops.mx_matmul(a, _export(8, 128))
    with pytest.raises(ValueError, match="not served"):
        ops.mx_matmul(_export(4, 96), _export(8, 96))           # a multiple of 32, not of the kernel's 128
    with pytest.raises(ValueError, match="2-D"):
        ops.mx_matmul(a, ops.MXExport(w.elements, w.scales, "mxfp4", (2, 4, 256), torch.float32))
    for bad in ("mxfp6_e2m3", "mxfp6_e3m2"):
        with pytest.raises(ValueError, match="FP6"):
            ops.mx_matmul(ops.MXExport(a.elements, a.scales, bad, a.shape, a.dtype), w)
        with pytest.raises(ValueError, match="FP6"):
            ops.mx_matmul(a, ops.MXExport(w.elements, w.scales, bad, w.shape, w.dtype))
    with pytest.raises(ValueError, match="unknown MX format"):
        ops.mx_matmul(ops.MXExport(a.elements, a.scales, "int4", a.shape, a.dtype), w)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.mx_matmul(a, w, out_dtype=torch.float64)
    for allow in (False, True):                                  # CPU tensors raise like the rest of the MX path
        llm_qat_amd.allow_cpu_tensors(allow)
        try:
            with pytest.raises(RuntimeError, match="no CPU"):
                ops.mx_matmul(a, w)
        finally:
            llm_qat_amd.allow_cpu_tensors(False)
    assert "mx_gemm_launch" not in llm_qat_amd.stats()


def test_fq_mx_gemm_validation_codes():
    L = _lib.lib()
    f = 1 << 20       # 16-byte-aligned non-NULL addresses: never dereferenced, validation fails first
    ok = dict(a_fmt=3, w_fmt=0, M=4, N=8, K=256, dt=_lib.DTYPE_BF16, ae=f, asc=f + 4096, we=f + 8192, wsc=f + 12288, out=f + 16384)

    def call(**kw):
        p = dict(ok, **kw)
        return L.fq_mx_gemm(p["ae"], p["asc"], p["a_fmt"], p["we"], p["wsc"], p["w_fmt"], p["out"], p["M"], p["N"], p["K"], p["dt"], None)

    assert call(dt=_lib.DTYPE_F64) == -1 and call(dt=9) == -1 and call(dt=-1) == -1
    for fmt in (1, 2, 5, -1):                                   # FP6 and unknown codes, either operand
        assert call(a_fmt=fmt) == -7 and call(w_fmt=fmt) == -7
    assert call(M=-1) == -3 and call(N=-1) == -3 and call(K=-128) == -3
    assert call(K=96) == -3 and call(K=32) == -3 and call(K=0) == -3          # K: a positive multiple of 128
    assert call(M=2 ** 31) == -3 and call(N=2 ** 40) == -3 and call(K=2 ** 31) == -3
    for p in ("ae", "asc", "we", "wsc", "out"):
        assert call(**{p: None}) == -4
    for p in ("ae", "we", "out"):
        assert call(**{p: f + 8}) == -8
    assert call(M=33, N=128 * 65535 + 1) == -8                                 # beyond one launch's grid
    assert call(M=0, ae=None, asc=None, out=None) == 0 and call(N=0, we=None, wsc=None, out=None) == 0   # empty: no launch
    assert b"" == L.fq_last_error()


def test_header_declares_fq_mx_gemm_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "llmqat_fakequant.h")).read()
    m = re.search(r"^int fq_mx_gemm\(([^;]*)\);", hdr, re.M | re.S)
    assert m, "fq_mx_gemm is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = ["p" if "*" in p else "q" if p.startswith("int64_t") else "i" for p in params]
    assert "".join(kinds) == "ppippipqqqip"                      # pointers, int, int64 and the stream only
    assert "fq_mx_gemm" in _lib.EXPORTS
    L = _lib.lib()
    import ctypes
    assert [("p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64 else "i") for t in L.fq_mx_gemm.argtypes] == kinds
    assert L.fq_version() == _lib.ABI_VERSION


def test_abi_fuzz_and_export_tests_pass_with_the_new_name():
    import test_abi_and_host as T
    T.test_library_exports_every_declared_symbol()
    T.test_abi_rejects_null_pointers_and_hostile_sizes_before_any_launch()


def test_mx_linear_eligibility_errors():
    F = MXLinear.from_quantize_linear
    with pytest.raises(ValueError, match="expected a QuantizeLinear"):
        F(torch.nn.Linear(256, 64))
    with pytest.raises(ValueError, match="weight_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8))                                           # integer-quantized
    with pytest.raises(ValueError, match="act_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_format="mxfp4"))
    with pytest.raises(ValueError, match="weight_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_group_size=32, act_format="mxfp8_e4m3"))   # group-wise weight
    with pytest.raises(ValueError, match="no export packing"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_format="mxfp6_e2m3", act_format="mxfp8_e4m3"))
    with pytest.raises(ValueError, match="in_features=96"):
        F(QuantizeLinear(96, 64, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3"))
    with pytest.raises(ValueError):
        MXLinear(96, 64)
    with pytest.raises(ValueError):
        MXLinear(256, 64, weight_format="mxfp6_e3m2")
    prev = llm_qat_amd.default_mx_formats("mxfp4", "mxfp8_e4m3")   # formats through the process default resolve too: only the device is missing
    try:
        layer = QuantizeLinear(256, 64, w_bits=4, a_bits=8)
    finally:
        llm_qat_amd.default_mx_formats(*prev)
    with pytest.raises(RuntimeError, match="no CPU"):
        F(layer)
    model = torch.nn.Sequential(QuantizeLinear(256, 64, w_bits=8, a_bits=8), torch.nn.Linear(64, 8),
                                QuantizeLinear(96, 64, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3"))
    kept = list(model)
    assert convert_to_mx_inference(model) == 0 and all(a is b for a, b in zip(model, kept))


def test_mx_linear_state_dict_round_trip_and_no_float_weight():
    torch.manual_seed(0)
    m = MXLinear(256, 64, "mxfp4", "mxfp8_e4m3", bias=True, dtype=torch.bfloat16)
    assert m.weight_elements.shape == (64, 128) and m.weight_scales.shape == (64, 8) and m.bias.shape == (64,)
    assert MXLinear(256, 64, "mxfp8_e5m2", "mxfp4").weight_elements.shape == (64, 256)
    assert list(m.parameters()) == [] and sorted(m.state_dict()) == ["bias", "weight_elements", "weight_scales"]
    m.weight_elements.copy_(torch.randint(0, 256, (64, 128), dtype=torch.uint8))
    m.weight_scales.copy_(torch.randint(100, 140, (64, 8), dtype=torch.uint8))
    m.bias.normal_()
    m2 = MXLinear(256, 64, "mxfp4", "mxfp8_e4m3", bias=True, dtype=torch.bfloat16)
    m2.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]) and v.dtype == m2.state_dict()[k].dtype
    assert sorted(MXLinear(256, 64).state_dict()) == ["weight_elements", "weight_scales"]
    with pytest.raises(RuntimeError):                                # a layer of another shape does not load
        MXLinear(512, 64).load_state_dict(m.state_dict())
    x = torch.zeros(2, 256, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m(x)


def test_reference_on_worked_values():
    """A row [1.5, -2, 0...] x 2^1 (block 0) and [6, 0.5, 0...] x 2^-2 (block 4), W rows with the matching elements: by hand."""
    K = 256
    av = np.zeros((1, K), np.float32)
    av[0, 0], av[0, 1], av[0, 128], av[0, 129] = 1.5, -2.0, 6.0, 0.5
    asc = np.full((1, K // 32), 127, np.uint8)
    asc[0, 0], asc[0, 4] = 128, 125
    wv = np.zeros((2, K), np.float32)
    wv[0, 0], wv[0, 1], wv[0, 128] = 4.0, 3.0, -1.0
    wv[1, 129], wv[1, 2] = -6.0, 6.0
    wsc = np.full((2, K // 32), 127, np.uint8)
    wsc[0, 0], wsc[0, 4], wsc[1, 4] = 126, 130, 0x7E
    for a_fmt in ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"):
        for w_fmt in ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"):
            a = export_from_codes(codes_of_values(av, a_fmt), asc, a_fmt)
            w = export_from_codes(codes_of_values(wv, w_fmt), wsc, w_fmt)
            ref, S = ref64(a, w)
            # out[0, 0] = (3 * 2 + -4 * 1.5) [block 0: A x2, W x0.5] + (1.5 * -8) [block 4: 6 x 2^-2 times -1 x 2^3] = 0 - 12
            # out[0, 1] = 0.5 * 2^-2 * -6 * 2^-1 = -0.375
            assert ref.tolist() == [[-12.0, -0.375]]
            assert S.tolist() == [[3 * 2 + 4 * 1.5 + 12.0, 0.375]]
    a.scales[0, 7] = 0xFF                                            # an 0xFF block anywhere in the row poisons the row
    assert torch.isnan(ref64(a, w)[0]).all()
    z = export_from_codes(np.full((1, K), 2, np.uint8), np.zeros((1, K // 32), np.uint8), "mxfp4")     # scale byte 0 is 2^-127
    big = export_from_codes(np.full((1, K), 2, np.uint8), np.full((1, K // 32), 254, np.uint8), "mxfp4")
    assert ref64(z, big)[0].item() == 256.0


def test_exactness_proof_rejects_inputs_that_could_round():
    rng = np.random.default_rng(0)
    a, ai = grid_operand(rng, 4, 4096, "mxfp4")
    w, wi = grid_operand(rng, 8, 4096, "mxfp8_e4m3")
    assert prove_exact(ai, wi) < 2 ** 24
    ref, _ = ref64(a, w)
    assert torch.equal(ref, torch.from_numpy((ai @ wi.T).astype(np.float64) * 0.25))
    with pytest.raises(AssertionError):
        prove_exact(ai * 64, wi)


def test_the_product_does_not_import_tools_or_oracle():
    src = open(os.path.join(ROOT, "llm-qat_amd", "mx_inference.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(tools|oracle)\b", src, re.M)
