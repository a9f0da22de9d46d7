"""The MX dequantize kernel (fqi_mx_dequant, ops.mx_dequantize) and MXLinear's dequantized route on the MI355X.
Every comparison is on bit patterns with zero tolerance (conftest.bits_equal's rule: any NaN equals any NaN).  The reference of the
kernel is ops.MXExport.dequantize() computed on CPU copies; the reference of the route is QuantizeLinear.eval().  The launch-tail sizes
come from the kernel's launch constants, read from csrc/fq_launch.h; the case sets from tests/mx_dequant_cases.py, whose sensitivity
tests/test_mx_dequant_cpu.py shows on the reference alone."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.mx_inference import MXLinear, convert_to_mx_inference
from llm_qat_amd.utils_quant import QuantizeLinear

from conftest import bits_equal, mismatch_report
import mx_dequant_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LAUNCH_H = open(os.path.join(ROOT, "llm-qat_amd", "csrc", "fq_launch.h")).read()
_m = re.search(r"constexpr int MX_TPB = (\d+), MX_VPT = (\d+);", _LAUNCH_H)
WG_VECS = int(_m.group(1)) * int(_m.group(2))            # 16-byte output vectors one workgroup covers
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}
RULES = ("floor", "ceil")


def assert_bits(got, want, dtype, what=""):
    g, w = C.bits(got, dtype), C.bits(want, dtype)
    if dtype == "fp32":
        g, w = g.view(np.float32), w.view(np.float32)
    assert g.shape == w.shape, (g.shape, w.shape)
    assert bits_equal(g, w, dtype), f"{what}: {mismatch_report(g, w, dtype)}"


def run(elements, scales, fmt, shape, dtype):
    return ops.mx_dequantize_tensors(elements.cuda(), scales.cuda(), fmt, shape, C.TDT[dtype])


# ---- every code under every scale byte ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exhaustive_reference(fmt, dtype):
    elements, scales, shape = C.exhaustive(fmt)
    return C.reference(elements, scales, fmt, shape, dtype)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("fmt", C.FMTS)
def test_every_code_under_every_scale_byte(fmt, dtype):
    elements, scales, shape = C.exhaustive(fmt)
    llm_qat_amd.stats(reset=True)
    got = run(elements, scales, fmt, shape, dtype)
    st = llm_qat_amd.stats()
    assert st.get("mx_dequant_launch") == 1 and "mx_copy_route" not in st, st
    assert got.shape == shape and got.dtype is C.TDT[dtype] and got.is_contiguous()
    assert_bits(got, _exhaustive_reference(fmt, dtype), dtype, f"{fmt} -> {dtype}")


# ---- round trip: mx_dequantize(mx_export(x)) == mx_quantize(x) --------------------------------------------------------------------------------

def _hard_input(shape, dtype, seed):
    """random values over many binades with a NaN block, an Inf block, an all-zero block and negative zeros (as far as the shape has room)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-20, 12, shape, generator=g).float())
    flat = x.reshape(-1, 32)
    nb = flat.shape[0]
    flat[0, 3] = -0.0
    flat[0, 4] = 0.0
    if nb >= 2:
        flat[1] = 0.0
        flat[1, 7] = -0.0
    if nb >= 3:
        flat[2, 5] = float("nan")
    if nb >= 4:
        flat[nb - 1, 31] = float("-inf")
    return x.to(C.TDT[dtype]).cuda()


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("fmt", C.FMTS)
def test_round_trip_gives_the_fake_quantized_tensor(fmt, dtype):
    for i, shape in enumerate(((1, 32), (3, 32), (5, 96), (4097, 96), (2, 3, 64))):
        x = _hard_input(shape, dtype, 100 + i)
        for rotate in ((False, True) if shape[-1] % 64 == 0 else (False,)):
            for rule in RULES:
                e = ops.mx_export(x, fmt, rotate=rotate, scale_rule=rule)
                want = ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=rule)
                got = ops.mx_dequantize(e)
                assert got.shape == x.shape and got.dtype is x.dtype
                assert_bits(got, want, dtype, f"{fmt} {dtype} {shape} rotate={rotate} {rule}")


def test_round_trip_dtype_overrides_and_a_square_weight():
    x = _hard_input((5, 96), "bf16", 7)
    e = ops.mx_export(x, "mxfp4")
    cpu = ops.MXExport(e.elements.cpu(), e.scales.cpu(), e.fmt, e.shape, torch.float32)
    for dtype in C.DTYPES:                              # a bf16 export read back in each dtype: the reference with that dtype
        got = ops.mx_dequantize(e, dtype=C.TDT[dtype])
        cpu.dtype = C.TDT[dtype]
        assert got.dtype is C.TDT[dtype]
        assert_bits(got, cpu.dequantize(), dtype, f"bf16 export as {dtype}")
    assert_bits(ops.mx_dequantize(e, dtype=torch.float32), ops.mx_quantize(x, "mxfp4").float(), "fp32", "bf16 export as fp32")
    x32 = _hard_input((3, 64), "fp32", 8)
    e32 = ops.mx_export(x32, "mxfp8_e5m2")               # an fp32 export read back as fp16: the fp32 result rounded once more
    assert_bits(ops.mx_dequantize(e32, dtype=torch.float16), ops.mx_quantize(x32, "mxfp8_e5m2").half(), "fp16", "fp32 export as fp16")
    w = (torch.randn(4096, 4096, generator=torch.Generator().manual_seed(9)) * 0.02).to(torch.bfloat16).cuda()
    ew = ops.mx_export(w, "mxfp4")
    want = ops.mx_quantize(w, "mxfp4")
    got = ops.mx_dequantize(ew)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_an_empty_export_launches_nothing():
    llm_qat_amd.stats(reset=True)
    for shape in ((0, 32), (4, 0), (2, 0, 64)):
        n = int(np.prod(shape))
        y = ops.mx_dequantize_tensors(torch.empty(n // 2, dtype=torch.uint8, device="cuda"), torch.empty(n // 32, dtype=torch.uint8, device="cuda"),
                                      "mxfp4", shape, torch.bfloat16)
        assert y.shape == shape and y.dtype is torch.bfloat16 and y.is_cuda
    assert "mx_dequant_launch" not in llm_qat_amd.stats()


# ---- launch tails: one block fewer than, exactly, and one block more than one and two workgroups cover -----------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("fmt", C.FMTS)
def test_launch_tails_around_one_and_two_workgroups(fmt, dtype):
    wg_blocks = WG_VECS * 16 // ESIZE[dtype] // 32        # blocks of 32 elements one workgroup covers
    assert wg_blocks * 32 * ESIZE[dtype] == WG_VECS * 16
    for k, nblocks in enumerate((wg_blocks - 1, wg_blocks, wg_blocks + 1, 2 * wg_blocks - 1, 2 * wg_blocks, 2 * wg_blocks + 1)):
        elements, scales, shape = C.random_export(nblocks, fmt, 40 + k)
        got = run(elements, scales, fmt, shape, dtype)
        assert_bits(got, C.reference(elements, scales, fmt, shape, dtype), dtype, f"{fmt} {dtype} {nblocks} blocks")


# ---- canaries: the C entry point writes y and nothing else -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("fmt", C.FMTS)
def test_canaries_around_y_and_inputs_unchanged(fmt, dtype):
    wg_blocks = WG_VECS * 16 // ESIZE[dtype] // 32
    nblocks = wg_blocks + 3                                # a second, partly filled workgroup
    elements, scales, shape = C.random_export(nblocks, fmt, 77)
    ybytes = nblocks * 32 * ESIZE[dtype]
    e, s = elements.cuda(), scales.cuda()
    buf = torch.full((64 + ybytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rc = ops._launch(e, _lib.lib().fqi_mx_dequant, e.data_ptr(), s.data_ptr(), buf.data_ptr() + 64, nblocks, 32, ops.MX_FORMATS[fmt],
                     ops._OUT_DTYPES[C.TDT[dtype]])
    _lib.check(rc, "fqi_mx_dequant")
    torch.cuda.synchronize()
    out = buf.cpu()
    assert (out[:64] == 0xA5).all() and (out[-64:] == 0xA5).all()
    got = out[64:-64].view(C.TDT[dtype]).reshape(shape)
    assert_bits(got, C.reference(elements, scales, fmt, shape, dtype), dtype, f"{fmt} {dtype}")
    assert torch.equal(e.cpu(), elements) and torch.equal(s.cpu(), scales)


# ---- the copy route ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", C.FMTS)
def test_copy_route_for_views_and_misaligned_buffers(fmt):
    elements, scales, shape = C.random_export(70, fmt, 5)
    want = C.reference(elements, scales, fmt, shape, "bf16")
    eb = elements.shape[1]
    wide = torch.zeros(70, 2 * eb, dtype=torch.uint8)
    wide[:, :eb] = elements
    view = wide.cuda()[:, :eb]                                             # a sliced, non-contiguous view
    assert not view.is_contiguous()
    off = torch.zeros(elements.numel() + 1, dtype=torch.uint8, device="cuda")
    off[1:] = elements.reshape(-1).cuda()
    shifted = off[1:].reshape(elements.shape)                              # contiguous, one byte off the alignment
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 1
    for e in (view, shifted):
        llm_qat_amd.stats(reset=True)
        got = ops.mx_dequantize_tensors(e, scales.cuda(), fmt, shape, torch.bfloat16)
        st = llm_qat_amd.stats()
        assert st.get("mx_copy_route") == 1 and st.get("mx_dequant_launch") == 1, st
        assert_bits(got, want, "bf16", fmt)
    sview = torch.stack((scales, scales), -1).cuda()[..., 0]               # the scales as a strided view: one copy too
    assert not sview.is_contiguous()
    llm_qat_amd.stats(reset=True)
    got = ops.mx_dequantize_tensors(elements.cuda(), sview, fmt, shape, torch.bfloat16)
    assert llm_qat_amd.stats().get("mx_copy_route") == 1
    assert_bits(got, want, "bf16", fmt)


def test_device_side_argument_errors():
    e = ops.mx_export(torch.randn(4, 64, device="cuda", dtype=torch.bfloat16), "mxfp4")
    with pytest.raises(RuntimeError, match="no CPU"):                       # either buffer on the CPU
        ops.mx_dequantize_tensors(e.elements, e.scales.cpu(), "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.mx_dequantize_tensors(e.elements.cpu(), e.scales.cpu(), "mxfp4", e.shape, torch.bfloat16)
    with pytest.raises(ValueError, match="elements holds"):
        ops.mx_dequantize_tensors(e.elements, e.scales, "mxfp8_e4m3", e.shape, torch.bfloat16)


# ---- MXLinear(dequant_above=0) against QuantizeLinear.eval() ----------------------------------------------------------------------------------

def _layer(weight_format, act_format, dtype, rotate, rule, bias, seed=0):
    torch.manual_seed(seed)
    layer = QuantizeLinear(256, 96, w_bits=4, a_bits=8, weight_format=weight_format, act_format=act_format, mx_rotate=rotate,
                           mx_scale_rule=rule).to("cuda", C.TDT[dtype])
    with torch.no_grad():
        layer.weight.mul_(3.0)
    if bias:                                               # (the constructor takes no bias, as the reference's: a trained one is assigned)
        layer.bias = torch.nn.Parameter((torch.randn(96) * 0.5).to("cuda", C.TDT[dtype]))
    return layer.eval()


PAIRS = (("mxfp4", "mxfp8_e4m3"), ("mxfp8_e5m2", "mxfp4"), ("mxfp8_e4m3", "mxfp8_e4m3"))


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("wf,af", PAIRS)
def test_mx_linear_dequant_route_equals_quantize_linear_eval(wf, af, dtype):
    for rotate in (False, True):
        for rule in RULES:
            for bias in (False, True):
                layer = _layer(wf, af, dtype, rotate, rule, bias)
                mxl = MXLinear.from_quantize_linear(layer, dequant_above=0)
                assert mxl.dequant_above == 0 and mxl.rotate is rotate and mxl.scale_rule == rule and (mxl.bias is not None) == bias
                for tokens in (1, 33, 64):
                    x = (torch.randn(tokens, 256, generator=torch.Generator().manual_seed(tokens)) * 2).to(C.TDT[dtype]).cuda()
                    x[0, 5] *= 40                                               # an outlier in one block
                    with torch.no_grad():
                        want = layer(x)
                        got = mxl(x)
                    assert got.shape == want.shape == (tokens, 96) and got.dtype is want.dtype
                    assert_bits(got, want, dtype, f"W {wf} A {af} {dtype} rotate={rotate} {rule} bias={bias} tokens={tokens}")


def test_mx_linear_dequant_route_on_a_batched_input():
    layer = _layer("mxfp4", "mxfp8_e4m3", "bf16", False, "floor", True)
    mxl = MXLinear.from_quantize_linear(layer, dequant_above=5)
    x = torch.randn(2, 3, 256, device="cuda", dtype=torch.bfloat16)         # 6 rows: above 5
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        got = mxl(x)
    assert llm_qat_amd.stats().get("mx_dequant_launch") == 1 and got.shape == (2, 3, 96)
    with torch.no_grad():
        want = layer(x.reshape(6, 256)).reshape(2, 3, 96)
    assert_bits(got, want, "bf16", "batched")


# ---- routing ----------------------------------------------------------------------------------------------------------------------------------

def _counts(m, x):
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        m(x)
    st = llm_qat_amd.stats()
    return {k: st.get(k, 0) for k in ("mx_launch", "mx_export_launch", "mx_gemm_launch", "mx_dequant_launch")}


def test_routing_by_the_number_of_rows():
    layer = _layer("mxfp4", "mxfp8_e4m3", "bf16", False, "floor", False)
    routed = MXLinear.from_quantize_linear(layer, dequant_above=32)
    plain = MXLinear.from_quantize_linear(layer)
    x32, x33, x64 = (torch.randn(n, 256, device="cuda", dtype=torch.bfloat16) for n in (32, 33, 64))
    assert _counts(routed, x32) == {"mx_launch": 0, "mx_export_launch": 1, "mx_gemm_launch": 1, "mx_dequant_launch": 0}
    assert _counts(routed, x33) == {"mx_launch": 1, "mx_export_launch": 0, "mx_gemm_launch": 0, "mx_dequant_launch": 1}
    assert _counts(plain, x64) == {"mx_launch": 0, "mx_export_launch": 1, "mx_gemm_launch": 1, "mx_dequant_launch": 0}
    assert plain.dequant_above is None
    # the state dict does not carry the argument: it loads both ways, and the routes stay the modules' own
    assert set(plain.state_dict()) == set(routed.state_dict())
    other = MXLinear(256, 96, "mxfp4", "mxfp8_e4m3", device="cuda", dequant_above=32)
    other.load_state_dict(plain.state_dict())
    back = MXLinear(256, 96, "mxfp4", "mxfp8_e4m3", device="cuda")
    back.load_state_dict(other.state_dict())
    with torch.no_grad():
        assert torch.equal(other(x33).view(torch.int16), routed(x33).view(torch.int16))
        assert torch.equal(back(x33).view(torch.int16), plain(x33).view(torch.int16))
    assert _counts(other, x33)["mx_dequant_launch"] == 1 and _counts(back, x33)["mx_dequant_launch"] == 0
    model = torch.nn.Sequential(_layer("mxfp4", "mxfp8_e4m3", "bf16", False, "floor", False))
    assert convert_to_mx_inference(model, dequant_above=7) == 1 and model[0].dequant_above == 7


# ---- torch.compile ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_mx_linear_dequant_route_compiles_fullgraph(backend):
    if backend == "inductor":
        try:
            import triton  # noqa: F401
        except ImportError:
            pytest.skip("inductor needs triton, which this environment does not have")
    torch._dynamo.reset()
    layer = _layer("mxfp4", "mxfp8_e4m3", "bf16", True, "ceil", False)
    mxl = MXLinear.from_quantize_linear(layer, dequant_above=0)
    x = torch.randn(48, 256, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        eager = mxl(x)
        llm_qat_amd.stats(reset=True)
        got = torch.compile(mxl, fullgraph=True, backend=backend)(x)
    st = llm_qat_amd.stats()
    assert st.get("mx_dequant_launch", 0) >= 1 and "mx_gemm_launch" not in st, st
    assert torch.equal(got.view(torch.int16), eager.view(torch.int16))
