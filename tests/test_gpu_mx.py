"""OCP MX block-scaled fake quantization on the MI355X: fq_mx_fwd / fq_mx_export against the numpy reference (tests/mx_reference.py),
zero tolerance on bits (any NaN equals any NaN); robustness (misaligned / transposed inputs, canaries); the identity gradient; and
QuantizeLinear(weight_format=, act_format=) against F.linear of reference-quantized operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_reference import decode, export_bits, pack_fp4, quantize_bits, quantize_values

pytestmark = pytest.mark.gpu

FMTS = ["mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e4m3", "mxfp8_e5m2"]
EXPORT_FMTS = ["mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"]
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}


def to_bits(t, dtype):
    return t.detach().contiguous().cpu().view(IDT[dtype]).numpy().view(NDT[dtype])


def from_bits(b, dtype, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16 if NDT[dtype] is np.uint16 else np.int32)).view(TDT[dtype]).to(device)


def assert_bits_equal(got, want, dtype):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    gn, wn = np.isnan(decode(got, dtype)), np.isnan(decode(want, dtype))
    assert np.array_equal(gn, wn), f"NaN positions differ: {np.flatnonzero(gn != wn)[:8]}"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{bad.size} elements differ, first {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}"


def exhaustive_bits(dtype):
    """every 16-bit pattern: finite ones in blocks led by a chosen amax (each block holds only patterns with |v| <= that amax), the
    non-finite ones in blocks of their own"""
    allb = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    v = decode(allb, dtype)
    fin = np.isfinite(v)
    lead = [1.0, 5.0, 7.5, 2.0 ** -126, 2.0 ** -133, 3e38, 0.1, 448.0, 1000.0, 65504.0, 6e-8] if dtype == "fp16" or dtype == "bf16" else []
    lead_bits = []
    for a in lead:
        t = torch.tensor([a], dtype=torch.float32).to(TDT[dtype])
        if not torch.isfinite(t).all() or t.item() == 0:
            continue
        lead_bits.append(int(t.view(torch.int16).item()) & 0xFFFF)
    blocks = []
    for lb in lead_bits:
        a = abs(decode(np.array([lb], np.uint16), dtype)[0])
        cand = allb[fin & (np.abs(v) <= a)]
        pad = (-len(cand)) % 31
        cand = np.concatenate([cand, np.zeros(pad, np.uint16)]).reshape(-1, 31)
        blocks.append(np.concatenate([np.full((len(cand), 1), lb, np.uint16), cand], 1))
    nonfin = allb[~fin]
    pad = (-len(nonfin)) % 32
    blocks.append(np.concatenate([nonfin, np.full(pad, 0x3F80 if dtype == "bf16" else 0x3C00, np.uint16)]).reshape(-1, 32))
    out = np.concatenate(blocks, 0)
    return out.reshape(-1, 256) if out.size % 256 == 0 else np.concatenate([out.reshape(-1), np.zeros((-out.size) % 256, np.uint16)]).reshape(-1, 256)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fwd_exhaustive_16bit(fmt, dtype):
    b = exhaustive_bits(dtype)
    y = ops.mx_quantize(from_bits(b, dtype), fmt)
    assert y.dtype is TDT[dtype] and y.shape == b.shape
    assert_bits_equal(to_bits(y, dtype), quantize_bits(b, dtype, fmt), dtype)


def rand_bits(shape, dtype, seed):
    """values over many binades, with zeros, signed zeros, subnormals and a few non-finite blocks"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-30, 30, shape[:-1] + (shape[-1] // 32, 1), generator=g).float()).repeat_interleave(32, -1).reshape(shape)
    x = x.to(TDT[dtype])
    flat = x.view(-1)
    n = flat.numel()
    idx = torch.randint(0, n, (max(1, n // 1000),), generator=g)
    flat[idx[: len(idx) // 3]] = -0.0
    flat[idx[len(idx) // 3: 2 * len(idx) // 3]] = torch.finfo(TDT[dtype]).tiny / 4
    flat[idx[-2:]] = float("nan")
    flat[idx[-3:-2]] = float("inf")
    return to_bits(x, dtype)


SHAPES = [(3, 32), (4097, 96), (2, 3, 4, 64), (4096, 11008), (11008, 4096), (2, 2048, 4096)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_fwd_small_shapes(fmt, dtype):
    for k, shape in enumerate(SHAPES[:3]):
        b = rand_bits(shape, dtype, 10 + k)
        y = ops.mx_quantize(from_bits(b, dtype), fmt)
        assert tuple(y.shape) == shape
        assert_bits_equal(to_bits(y, dtype), quantize_bits(b, dtype, fmt), dtype)


@pytest.mark.parametrize("shape,dtype,fmt", [(SHAPES[3], "bf16", "mxfp4"), (SHAPES[4], "bf16", "mxfp4"), (SHAPES[5], "bf16", "mxfp4"),
                                             (SHAPES[3], "bf16", "mxfp8_e4m3"), (SHAPES[3], "fp16", "mxfp6_e3m2"), (SHAPES[5], "fp32", "mxfp8_e5m2")])
def test_fwd_model_shapes(shape, dtype, fmt):
    b = rand_bits(shape, dtype, 20)
    y = ops.mx_quantize(from_bits(b, dtype), fmt)
    assert_bits_equal(to_bits(y, dtype), quantize_bits(b, dtype, fmt), dtype)


@pytest.mark.parametrize("fmt", EXPORT_FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_export_matches_reference_and_forward(fmt, dtype):
    for k, shape in enumerate([(3, 32), (4097, 96), (2, 3, 4, 64), (512, 4096)]):
        b = rand_bits(shape, dtype, 30 + k)
        x = from_bits(b, dtype)
        e = ops.mx_export(x, fmt)
        cols = shape[-1]
        assert e.elements.dtype is torch.uint8 and tuple(e.elements.shape) == shape[:-1] + (cols // 2 if fmt == "mxfp4" else cols,)
        assert tuple(e.scales.shape) == shape[:-1] + (cols // 32,)
        codes, scales = export_bits(b, dtype, fmt)
        assert np.array_equal(e.scales.cpu().numpy().reshape(-1), scales)
        want = pack_fp4(codes) if fmt == "mxfp4" else codes
        assert np.array_equal(e.elements.cpu().numpy().reshape(-1), want)
        y = ops.mx_quantize(x, fmt)
        assert_bits_equal(to_bits(e.dequantize(), dtype), to_bits(y, dtype), dtype)      # signed zeros included
        if fmt != "mxfp4":   # the codes decoded through torch's own float8 view, times the scales through float8_e8m0fnu: the reference values
            f8 = torch.float8_e4m3fn if fmt == "mxfp8_e4m3" else torch.float8_e5m2
            q = e.elements.view(f8).float().cpu().double().numpy().reshape(-1, 32)
            s = e.scales.view(torch.float8_e8m0fnu).float().cpu().double().numpy().reshape(-1)
            fin = scales != 0xFF
            assert np.array_equal(np.isnan(s), ~fin)
            assert np.array_equal((q * s[:, None])[fin], quantize_values(b, dtype, fmt).reshape(-1, 32)[fin])


def test_misaligned_and_transposed_inputs_take_one_copy():
    x = (torch.randn(64 * 128 + 8, device="cuda") * 3).bfloat16()
    v = x.view(-1)[1:1 + 64 * 128].view(64, 128)          # 2-byte offset: not 16-byte aligned
    assert v.data_ptr() % 16
    llm_qat_amd.stats(reset=True)
    y = ops.mx_quantize(v, "mxfp4")
    assert llm_qat_amd.stats().get("mx_copy_route") == 1
    assert torch.equal(y.view(torch.int16), ops.mx_quantize(v.clone(), "mxfp4").view(torch.int16))
    w = (torch.randn(128, 96, device="cuda")).half()
    wt = w.t()
    llm_qat_amd.stats(reset=True)
    e = ops.mx_export(wt, "mxfp8_e4m3")
    assert llm_qat_amd.stats().get("mx_copy_route") == 1 and llm_qat_amd.stats().get("mx_export_launch") == 1
    ref = ops.mx_export(wt.contiguous(), "mxfp8_e4m3")
    assert torch.equal(e.elements, ref.elements) and torch.equal(e.scales, ref.scales)
    assert_bits_equal(to_bits(ops.mx_quantize(wt, "mxfp8_e4m3"), "fp16"), quantize_bits(to_bits(wt, "fp16"), "fp16", "mxfp8_e4m3"), "fp16")


def test_canaries_untouched():
    """y, elements and scales written into the middle of larger buffers: the bytes around them keep their canary value"""
    from llm_qat_amd import _lib
    L = _lib.lib()
    for dtype, fmt in (("bf16", "mxfp4"), ("fp32", "mxfp8_e5m2"), ("fp16", "mxfp8_e4m3")):
        rows, cols = 37, 160
        b = rand_bits((rows, cols), dtype, 40)
        x = from_bits(b, dtype)
        es = x.element_size()
        pad = 256
        ybuf = torch.full((rows * cols * es + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
        code, dt = ops.MX_FORMATS[fmt], ops._DTYPES[x.dtype]
        assert L.fq_mx_fwd(x.data_ptr(), ybuf.data_ptr() + pad, rows, cols, code, dt, None) == 0
        nel = rows * cols // (2 if fmt == "mxfp4" else 1)
        ebuf = torch.full((nel + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda")
        sbuf = torch.full((rows * cols // 32 + 2 * pad,), 0x3C, dtype=torch.uint8, device="cuda")
        assert L.fq_mx_export(x.data_ptr(), ebuf.data_ptr() + pad, sbuf.data_ptr() + pad, rows, cols, code, dt, None) == 0
        torch.cuda.synchronize()
        for buf, val, n in ((ybuf, 0xA5, rows * cols * es), (ebuf, 0x5A, nel), (sbuf, 0x3C, rows * cols // 32)):
            assert (buf[:pad] == val).all() and (buf[pad + n:] == val).all()
        y = ybuf[pad: pad + rows * cols * es].view(x.dtype).view(rows, cols)
        assert_bits_equal(to_bits(y, dtype), quantize_bits(b, dtype, fmt), dtype)


def test_autograd_identity_nothing_saved_no_backward_launch():
    x = (torch.randn(8, 256, device="cuda") * 4).bfloat16().requires_grad_(True)
    saved = []
    llm_qat_amd.stats(reset=True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = llm_qat_amd.mx_quantize(x, "mxfp4")
    assert saved == []
    assert torch.equal(y.view(torch.int16), ops.mx_quantize(x.detach(), "mxfp4").view(torch.int16))
    g = torch.randn_like(y)
    llm_qat_amd.stats(reset=True)
    (gx,) = torch.autograd.grad(y, x, g)
    assert torch.equal(gx.view(torch.int16), g.view(torch.int16))
    assert llm_qat_amd.stats().get("mx_launch", 0) == 0


def ref_q(t, fmt):
    """reference-quantized tensor, as a torch tensor of t's dtype (built from the numpy reference's bits)"""
    dtype = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[t.dtype]
    return from_bits(quantize_bits(to_bits(t, dtype), dtype, fmt).reshape(tuple(t.shape)), dtype, t.device).view(tuple(t.shape))


def linear_case(master_fp32):
    torch.manual_seed(5)
    m = QuantizeLinear(256, 192, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3").cuda()
    with torch.no_grad():
        m.weight.mul_(3)
    if not master_fp32:
        m = m.bfloat16()
    x = (torch.randn(2, 64, 256, device="cuda") * 2).bfloat16().requires_grad_(True)
    g = torch.randn(2, 64, 192, device="cuda").bfloat16()
    return m, x, g


def reference_step(m, x, g, autocast):
    w = m.weight.detach().clone().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)

    class STE(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, fmt):
            return ref_q(t, fmt)

        @staticmethod
        def backward(ctx, go):
            return go, None
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        out = F.linear(STE.apply(xr, "mxfp8_e4m3"), STE.apply(w, "mxfp4"))
    out.backward(g)
    return out.detach(), xr.grad, w.grad


def module_step(m, x, g, autocast, fn=None):
    m.weight.grad = None
    xx = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        out = (m if fn is None else fn)(xx)
    out.backward(g)
    return out.detach(), xx.grad, m.weight.grad


def assert_same(a, b):
    for u, v in zip(a, b):
        assert u.dtype is v.dtype and u.shape == v.shape
        assert torch.equal(u.view(torch.int16 if u.element_size() == 2 else torch.int32), v.view(torch.int16 if v.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("master_fp32", [False, True])
def test_quantize_linear_matches_reference(master_fp32):
    m, x, g = linear_case(master_fp32)
    llm_qat_amd.stats(reset=True)
    xx = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=master_fp32):
        out = m(xx)
    st = llm_qat_amd.stats(reset=True)
    assert st.get("mx_launch") == 2 and not st.get("pair_launch") and not st.get("cpp_pair_forward")
    out.backward(g)
    st = llm_qat_amd.stats()
    assert st.get("mx_launch", 0) == 0
    assert_same((out.detach(), xx.grad, m.weight.grad), reference_step(m, x, g, master_fp32))


def test_quantize_linear_checkpointing():
    from torch.utils.checkpoint import checkpoint
    m, x, g = linear_case(False)
    got = module_step(m, x, g, False, fn=lambda t: checkpoint(m, t, use_reentrant=False))
    assert_same(got, reference_step(m, x, g, False))


@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_quantize_linear_compiled(backend):
    if backend == "inductor":
        try:
            import triton  # noqa: F401
        except ImportError:
            pytest.skip("inductor needs triton, which this environment does not have")
    torch._dynamo.reset()
    m, x, g = linear_case(False)
    cm = torch.compile(m, fullgraph=True, backend=backend)
    assert_same(module_step(m, x, g, False, fn=cm), reference_step(m, x, g, False))


def test_export_weight_round_trip():
    m, _, _ = linear_case(False)
    e = m.export_weight()
    assert isinstance(e, ops.MXExport) and e.fmt == "mxfp4" and e.shape == (192, 256)
    assert torch.equal(e.dequantize().view(torch.int16), ops.mx_quantize(m.weight.detach(), "mxfp4").view(torch.int16))
    m8 = QuantizeLinear(256, 64, w_bits=8, weight_format="mxfp8_e5m2").cuda().bfloat16()
    e8 = m8.export_weight()
    assert torch.equal(e8.dequantize().view(torch.int16), ops.mx_quantize(m8.weight.detach(), "mxfp8_e5m2").view(torch.int16))


def test_default_formats_reach_unchanged_model_code():
    prev = llm_qat_amd.default_mx_formats(weight="mxfp4", act="mxfp8_e4m3")
    try:
        m = QuantizeLinear(256, 192, bias=False, w_bits=4, a_bits=8).cuda().bfloat16()   # the reference's constructor call
    finally:
        llm_qat_amd.default_mx_formats(*prev)
    x = torch.randn(4, 256, device="cuda").bfloat16()
    llm_qat_amd.stats(reset=True)
    out = m(x)
    assert llm_qat_amd.stats().get("mx_launch") == 2
    assert torch.equal(out, F.linear(ref_q(x, "mxfp8_e4m3"), ref_q(m.weight.detach(), "mxfp4")))
