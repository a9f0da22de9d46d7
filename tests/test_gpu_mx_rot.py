"""The block-Hadamard rotation fused into the MX kernels, on the MI355X: fq_block_rotate / fq_mx_fwd_rot / fq_mx_export_rot against the
numpy reference (tests/mx_rot_reference.py over tests/mx_reference.py), zero tolerance on bits (any NaN equals any NaN); robustness
(misaligned / transposed inputs, canaries); the gradient grad R with nothing saved; QuantizeLinear(mx_rotate=True) against F.linear of
reference operands and the reference rotation of its operand gradients; MXLinear(rotate=True) under the fp32 accumulation bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import MXLinear, convert_to_mx_inference, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_reference import decode, encode, export_bits, pack_fp4, quantize_values
from mx_rot_reference import export_rot_bits, quantize_rot_bits, rotate_bits, rotate_values

pytestmark = pytest.mark.gpu

FMTS = ["mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e4m3", "mxfp8_e5m2"]
EXPORT_FMTS = ["mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"]
DTYPES = ["bf16", "fp16", "fp32"]
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
NAME = {v: k for k, v in TDT.items()}
U = 2.0 ** -24


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


def rand_bits(shape, dtype, seed):
    """values over many binades (one per 64-run, so runs mix magnitudes within a factor of a few), with zeros, signed zeros, subnormals
    and a few non-finite elements"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-30, 30, shape[:-1] + (shape[-1] // 64, 1), generator=g).float()).repeat_interleave(64, -1).reshape(shape)
    x = x.to(TDT[dtype])
    flat = x.view(-1)
    n = flat.numel()
    idx = torch.randint(0, n, (max(3, n // 1000),), generator=g)
    flat[idx[: len(idx) // 3]] = -0.0
    flat[idx[len(idx) // 3: 2 * len(idx) // 3]] = torch.finfo(TDT[dtype]).tiny / 4
    flat[idx[-2:]] = float("nan")
    flat[idx[-3:-2]] = float("inf")
    return to_bits(x, dtype)


def check_all_three(b, dtype, fmts, export_fmts, rot=None):
    """fq_block_rotate, fq_mx_fwd_rot for fmts and fq_mx_export_rot for export_fmts on the tensor with bit patterns b"""
    shape = b.shape
    x = from_bits(b, dtype)
    r = rotate_values(b, dtype) if rot is None else rot
    y = ops.mx_rotate(x)
    assert y.dtype is TDT[dtype] and tuple(y.shape) == shape
    assert_bits_equal(to_bits(y, dtype), encode(r.astype(np.float64), dtype), dtype)
    r32 = r.view(np.uint32)
    for fmt in fmts:
        q = ops.mx_quantize(x, fmt, rotate=True)
        assert q.dtype is TDT[dtype] and tuple(q.shape) == shape
        assert_bits_equal(to_bits(q, dtype), encode(quantize_values(r32, "fp32", fmt), dtype), dtype)
    for fmt in export_fmts:
        e = ops.mx_export(x, fmt, rotate=True)
        cols = shape[-1]
        assert e.rotated is True and e.fmt == fmt and e.shape == tuple(shape) and e.dtype is TDT[dtype]
        assert e.elements.dtype is torch.uint8 and tuple(e.elements.shape) == shape[:-1] + (cols // 2 if fmt == "mxfp4" else cols,)
        assert tuple(e.scales.shape) == shape[:-1] + (cols // 32,)
        codes, scales = export_bits(r32, "fp32", fmt)
        assert np.array_equal(e.scales.cpu().numpy().reshape(-1), scales)
        assert np.array_equal(e.elements.cpu().numpy().reshape(-1), pack_fp4(codes) if fmt == "mxfp4" else codes)
        # dequantize() of the rotated export is the rotated forward, bit for bit (signed zeros included)
        assert_bits_equal(to_bits(e.dequantize(), dtype), to_bits(ops.mx_quantize(x, fmt, rotate=True), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_shapes_all_formats(dtype):
    for k, shape in enumerate([(3, 64), (4097, 192), (2, 3, 4, 128)]):
        check_all_three(rand_bits(shape, dtype, 10 + k), dtype, FMTS, EXPORT_FMTS)


@pytest.mark.parametrize("shape,dtype,fmts,export_fmts", [
    ((4096, 11008), "bf16", ["mxfp4", "mxfp8_e4m3"], ["mxfp4"]),
    ((11008, 4096), "fp16", ["mxfp6_e3m2", "mxfp6_e2m3"], ["mxfp8_e4m3"]),
    ((2, 2048, 4096), "fp32", ["mxfp8_e5m2"], ["mxfp8_e5m2"]),
])
def test_model_shapes(shape, dtype, fmts, export_fmts):
    check_all_three(rand_bits(shape, dtype, 20), dtype, fmts, export_fmts)


def special_runs(dtype):
    """one 64-run per row: NaN, +-Inf, +-0, all-zero, magnitudes whose sums overflow (fp32 range for bf16 / fp32, the fp16 range at the
    final rounding), 16-bit subnormals, alternating signs that cancel, a lone outlier, and the largest finite value"""
    t = TDT[dtype]
    fi = torch.finfo(t)
    rows = []

    def run(fill=0.0):
        r = torch.full((64,), fill, dtype=torch.float32)
        rows.append(r)
        return r
    run()[17] = float("nan")
    run(1.0)[40] = float("inf")
    run(1.0)[3] = float("-inf")
    r = run(1.0); r[1] = float("inf"); r[2] = float("-inf")
    run()
    run(-0.0)
    r = run(); r[::2] = -0.0
    run(fi.max)
    run(-fi.max)
    r = run(fi.max); r[1::2] = -fi.max
    r = run(fi.max / 2); r[5] = -fi.max
    run(fi.max / 64)
    run(fi.max / 8)
    run(fi.tiny / 4)                       # subnormals of the dtype
    r = run(fi.tiny / 8); r[1::2] = -fi.tiny / 8
    r = run(fi.tiny); r[7] = fi.tiny / 2 ** 6
    run(fi.smallest_subnormal if hasattr(fi, "smallest_subnormal") else fi.tiny / 128)
    r = run(); r[63] = fi.max
    r = run(); r[0] = 6.0; r[32] = -0.2
    r = run(1.0); r[1::2] = -1.0
    r = run(0.3); r[31] = 300.0
    g = torch.Generator().manual_seed(3)
    rows.append(torch.randn(64, generator=g) * 1e30 if dtype != "fp16" else torch.randn(64, generator=g) * 3e4)
    rows.append(torch.randn(64, generator=g) * (1e-38 if dtype != "fp16" else 1e-6))
    x = torch.stack(rows).to(t)
    return torch.cat([x, x.flip(0)], 1).contiguous()   # two runs per row: a bad run must not reach its neighbour


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype):
    x = special_runs(dtype)
    b = to_bits(x, dtype)
    r = rotate_values(b, dtype)
    assert np.isnan(r).any() and np.isinf(r).any()      # the cases do what they say: NaN runs, and sums that overflowed
    check_all_three(b, dtype, FMTS, EXPORT_FMTS, rot=r)


def test_rotation_is_its_own_inverse_on_integer_data():
    x = torch.randint(-256, 257, (512, 1024), device="cuda").float()
    for t in (torch.float32, torch.bfloat16, torch.float16):
        xt = torch.randint(-8, 9, (512, 1024), device="cuda").to(t) if t is not torch.float32 else x
        assert torch.equal(ops.mx_rotate(ops.mx_rotate(xt)), xt)


def test_misaligned_and_transposed_inputs_take_one_copy():
    x = (torch.randn(64 * 128 + 8, device="cuda") * 3).bfloat16()
    v = x.view(-1)[1:1 + 64 * 128].view(64, 128)          # 2-byte offset: not 16-byte aligned
    assert v.data_ptr() % 16
    for call, counter in ((lambda t: ops.mx_quantize(t, "mxfp4", rotate=True), "mx_launch"), (ops.mx_rotate, "mx_rotate_launch")):
        llm_qat_amd.stats(reset=True)
        y = call(v)
        st = llm_qat_amd.stats()
        assert st.get("mx_copy_route") == 1 and st.get(counter) == 1
        assert torch.equal(y.view(torch.int16), call(v.clone()).view(torch.int16))
    assert_bits_equal(to_bits(ops.mx_quantize(v, "mxfp4", rotate=True), "bf16"), quantize_rot_bits(to_bits(v, "bf16"), "bf16", "mxfp4"), "bf16")
    w = (torch.randn(128, 192, device="cuda")).half()
    wt = w.t()                                            # [192, 128]
    llm_qat_amd.stats(reset=True)
    e = ops.mx_export(wt, "mxfp8_e4m3", rotate=True)
    st = llm_qat_amd.stats()
    assert st.get("mx_copy_route") == 1 and st.get("mx_export_launch") == 1 and "mx_rotate_launch" not in st
    ref = ops.mx_export(wt.contiguous(), "mxfp8_e4m3", rotate=True)
    assert torch.equal(e.elements, ref.elements) and torch.equal(e.scales, ref.scales)
    assert_bits_equal(to_bits(ops.mx_rotate(wt), "fp16"), rotate_bits(to_bits(wt, "fp16"), "fp16"), "fp16")


def test_counters_show_up_only_when_non_zero():
    x = torch.randn(4, 128, device="cuda").bfloat16()
    llm_qat_amd.stats(reset=True)
    assert "mx_rotate_launch" not in llm_qat_amd.stats()
    ops.mx_rotate(x)
    ops.mx_quantize(x, "mxfp4", rotate=True)
    ops.mx_export(x, "mxfp4", rotate=True)
    st = llm_qat_amd.stats(reset=True)
    assert (st.get("mx_rotate_launch"), st.get("mx_launch"), st.get("mx_export_launch")) == (1, 1, 1)
    assert "mx_rotate_launch" not in llm_qat_amd.stats()


def test_canaries_untouched():
    """y, elements and scales written into the middle of larger buffers: the bytes around them keep their canary value"""
    from llm_qat_amd import _lib
    L = _lib.lib()
    for dtype, fmt in (("bf16", "mxfp4"), ("fp32", "mxfp8_e5m2"), ("fp16", "mxfp8_e4m3")):
        rows, cols = 37, 192          # 37 * 192 / 8 = 888 vectors: the last workgroup is partly out of range
        b = rand_bits((rows, cols), dtype, 40)
        x = from_bits(b, dtype)
        es = x.element_size()
        pad = 256
        code, dt = ops.MX_FORMATS[fmt], ops._DTYPES[x.dtype]
        ybuf = torch.full((rows * cols * es + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
        rbuf = torch.full((rows * cols * es + 2 * pad,), 0xC3, dtype=torch.uint8, device="cuda")
        assert L.fq_mx_fwd_rot(x.data_ptr(), ybuf.data_ptr() + pad, rows, cols, code, dt, None) == 0
        assert L.fq_block_rotate(x.data_ptr(), rbuf.data_ptr() + pad, rows, cols, dt, None) == 0
        nel = rows * cols // (2 if fmt == "mxfp4" else 1)
        ebuf = torch.full((nel + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda")
        sbuf = torch.full((rows * cols // 32 + 2 * pad,), 0x3C, dtype=torch.uint8, device="cuda")
        assert L.fq_mx_export_rot(x.data_ptr(), ebuf.data_ptr() + pad, sbuf.data_ptr() + pad, rows, cols, code, dt, None) == 0
        torch.cuda.synchronize()
        for buf, val, n in ((ybuf, 0xA5, rows * cols * es), (rbuf, 0xC3, rows * cols * es), (ebuf, 0x5A, nel), (sbuf, 0x3C, rows * cols // 32)):
            assert (buf[:pad] == val).all() and (buf[pad + n:] == val).all()
        y = ybuf[pad: pad + rows * cols * es].view(x.dtype).view(rows, cols)
        assert_bits_equal(to_bits(y, dtype), quantize_rot_bits(b, dtype, fmt), dtype)
        r = rbuf[pad: pad + rows * cols * es].view(x.dtype).view(rows, cols)
        assert_bits_equal(to_bits(r, dtype), rotate_bits(b, dtype), dtype)
        codes, scales = export_rot_bits(b, dtype, fmt)
        assert np.array_equal(sbuf[pad: pad + rows * cols // 32].cpu().numpy(), scales)
        assert np.array_equal(ebuf[pad: pad + nel].cpu().numpy(), pack_fp4(codes) if fmt == "mxfp4" else codes)


def ref_rot(t):
    """the reference rotation of a tensor, as a torch tensor of t's dtype and device"""
    dtype = NAME[t.dtype]
    return from_bits(rotate_bits(to_bits(t, dtype), dtype).reshape(tuple(t.shape)), dtype, t.device).view(tuple(t.shape))


def ref_qrot(t, fmt):
    dtype = NAME[t.dtype]
    return from_bits(quantize_rot_bits(to_bits(t, dtype), dtype, fmt).reshape(tuple(t.shape)), dtype, t.device).view(tuple(t.shape))


def same_bits(a, b):
    return a.dtype is b.dtype and a.shape == b.shape and torch.equal(a.view(IDT[NAME[a.dtype]]), b.view(IDT[NAME[b.dtype]]))


def test_gradient_is_the_rotated_gradient_nothing_saved():
    x = (torch.randn(8, 256, device="cuda") * 4).bfloat16().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = llm_qat_amd.mx_quantize(x, "mxfp4", rotate=True)
        z = llm_qat_amd.block_rotate(x)
    assert saved == []
    assert same_bits(y, ref_qrot(x.detach(), "mxfp4")) and same_bits(z, ref_rot(x.detach()))
    g = torch.randn_like(y)
    llm_qat_amd.stats(reset=True)
    (gx,) = torch.autograd.grad(y, x, g)
    st = llm_qat_amd.stats(reset=True)
    assert st.get("mx_rotate_launch") == 1 and "mx_launch" not in st
    assert same_bits(gx, ref_rot(g))
    (gz,) = torch.autograd.grad(z, x, g)
    assert llm_qat_amd.stats().get("mx_rotate_launch") == 1
    assert same_bits(gz, ref_rot(g))
    xf = torch.randn(4, 128, device="cuda", requires_grad=True)        # fp32, and the unrotated form is untouched
    (gf,) = torch.autograd.grad(llm_qat_amd.mx_quantize(xf, "mxfp8_e4m3", rotate=True), xf, torch.ones_like(xf))
    assert same_bits(gf, ref_rot(torch.ones_like(xf)))
    (gi,) = torch.autograd.grad(llm_qat_amd.mx_quantize(xf, "mxfp8_e4m3"), xf, torch.ones_like(xf))
    assert torch.equal(gi, torch.ones_like(xf))


def linear_case(master_fp32):
    torch.manual_seed(5)
    m = QuantizeLinear(256, 192, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=True).cuda()
    with torch.no_grad():
        m.weight.mul_(3)
    if not master_fp32:
        m = m.bfloat16()
    x = (torch.randn(2, 64, 256, device="cuda") * 2).bfloat16()
    x[0, 3, 70] = 60.0                        # outliers, so that the rotation matters
    x[1, :, 131] *= 25
    g = torch.randn(2, 64, 192, device="cuda").bfloat16()
    return m, x.requires_grad_(True), g


class _RefRotSTE(torch.autograd.Function):
    """Q(t R) from the numpy reference; the gradient is the reference rotation of the incoming one"""

    @staticmethod
    def forward(ctx, t, fmt):
        return ref_qrot(t, fmt)

    @staticmethod
    def backward(ctx, go):
        return ref_rot(go), None


def reference_step(m, x, g, autocast):
    w = m.weight.detach().clone().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        out = F.linear(_RefRotSTE.apply(xr, "mxfp8_e4m3"), _RefRotSTE.apply(w, "mxfp4"))
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
        assert same_bits(u, v)


@pytest.mark.parametrize("master_fp32", [False, True])
def test_quantize_linear_matches_reference(master_fp32):
    m, x, g = linear_case(master_fp32)
    llm_qat_amd.stats(reset=True)
    xx = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16, enabled=master_fp32):
        out = m(xx)
    st = llm_qat_amd.stats(reset=True)
    assert st.get("mx_launch") == 2 and "mx_rotate_launch" not in st and not st.get("pair_launch") and not st.get("cpp_pair_forward")
    out.backward(g)
    st = llm_qat_amd.stats()
    assert st.get("mx_rotate_launch") == 2 and st.get("mx_launch", 0) == 0
    want = reference_step(m, x, g, master_fp32)
    assert_same((out.detach(), xx.grad, m.weight.grad), want)
    # and the rotation does what it is for: the layer's function is that of the unrotated operands, up to quantization error
    plain = F.linear(x.detach().float(), m.weight.detach().float())
    err_rot = (want[0].float() - plain).norm() / plain.norm()
    assert err_rot < 0.2


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
    f = torch.compile(lambda t: llm_qat_amd.block_rotate(llm_qat_amd.mx_quantize(t, "mxfp4", rotate=True)), fullgraph=True, backend=backend)
    xx = x.detach().clone().requires_grad_(True)
    y = f(xx)
    assert same_bits(y.detach(), ref_rot(ref_qrot(x.detach(), "mxfp4")))
    y.backward(torch.ones_like(y))
    assert same_bits(xx.grad, ref_rot(ref_rot(torch.ones_like(y))))


def test_export_weight_is_the_rotated_export_and_default_reaches_unchanged_model_code():
    m, _, _ = linear_case(False)
    e = m.export_weight()
    assert isinstance(e, ops.MXExport) and e.rotated and e.fmt == "mxfp4" and e.shape == (192, 256)
    assert same_bits(e.dequantize(), ref_qrot(m.weight.detach(), "mxfp4"))
    prev = llm_qat_amd.default_mx_formats(weight="mxfp4", act="mxfp8_e4m3")
    prev_rot = llm_qat_amd.default_mx_rotate(True)
    try:
        d = QuantizeLinear(256, 192, bias=False, w_bits=4, a_bits=8).cuda().bfloat16()   # the reference's constructor call
    finally:
        llm_qat_amd.default_mx_formats(*prev)
        llm_qat_amd.default_mx_rotate(prev_rot)
    x = torch.randn(4, 256, device="cuda").bfloat16()
    llm_qat_amd.stats(reset=True)
    out = d(x)
    assert llm_qat_amd.stats().get("mx_launch") == 2
    assert torch.equal(out, F.linear(ref_qrot(x, "mxfp8_e4m3"), ref_qrot(d.weight.detach(), "mxfp4")))


def cpu_export(e):
    return ops.MXExport(e.elements.cpu(), e.scales.cpu(), e.fmt, e.shape, torch.float32, e.rotated)


def test_mx_matmul_refuses_mismatched_rotation():
    x = torch.randn(8, 256, device="cuda").bfloat16()
    w = torch.randn(16, 256, device="cuda").bfloat16()
    for ra, rw in ((True, False), (False, True)):
        with pytest.raises(ValueError, match="rotat"):
            ops.mx_matmul(ops.mx_export(x, "mxfp8_e4m3", rotate=ra), ops.mx_export(w, "mxfp4", rotate=rw))
    out = ops.mx_matmul(ops.mx_export(x, "mxfp8_e4m3", rotate=True), ops.mx_export(w, "mxfp4", rotate=True), out_dtype=torch.float32)
    assert out.shape == (8, 16)


@pytest.mark.parametrize("tokens", [16, 512])
def test_mx_linear_rotated_within_the_fp32_accumulation_bound(tokens):
    """|out - ref| <= 2 K 2^-24 S (the bound of tests/test_gpu_mx_gemm.py) against the float64 product of the two rotated dequantize()
    results, and against the product of the eval() fake-quant layer's operands taken as fp32"""
    K, N = 4096, 1024
    torch.manual_seed(0)
    layer = QuantizeLinear(K, N, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=True).to("cuda", torch.bfloat16)
    x = torch.randn(tokens, K, device="cuda", dtype=torch.bfloat16)
    x[:, 5::128] *= 30                                     # outlier channels
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)     # a trained layer: two steps through the rotated backward
    for _ in range(2):
        opt.zero_grad()
        layer(x).float().square().mean().backward()
        opt.step()
    layer.eval()
    mxl = MXLinear.from_quantize_linear(layer)
    assert mxl.rotate is True and "rotate=True" in mxl.extra_repr()
    model = torch.nn.Sequential(layer)
    assert convert_to_mx_inference(model) == 1 and model[0].rotate is True
    assert torch.equal(model[0].weight_elements, mxl.weight_elements) and torch.equal(model[0].weight_scales, mxl.weight_scales)
    we = layer.export_weight()
    assert torch.equal(we.elements, mxl.weight_elements) and torch.equal(we.scales, mxl.weight_scales) and mxl.weight_export().rotated
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        y = mxl(x)
    st = llm_qat_amd.stats()
    assert st.get("mx_export_launch") == 1 and st.get("mx_gemm_launch") == 1 and "mx_launch" not in st and "mx_rotate_launch" not in st
    assert y.dtype is torch.bfloat16 and y.shape == (tokens, N)
    a = ops.mx_export(x, "mxfp8_e4m3", rotate=True)
    A, W = cpu_export(a).dequantize().double(), cpu_export(we).dequantize().double()
    ref, S = A @ W.T, A.abs() @ W.abs().T
    out32 = ops.mx_matmul(a, we, out_dtype=torch.float32)
    ratio = ((out32.cpu().double() - ref).abs() / (U * S).clamp_min(1e-300)).max().item()
    print(f"[mx_rot MXLinear tokens={tokens}] max |out - ref| / (2^-24 S) = {ratio:.4f}  (bound {2 * K})")
    assert ratio <= 2 * K
    assert torch.equal(y.view(torch.int16), out32.to(torch.bfloat16).view(torch.int16))    # the 16-bit output is the one rounding of that sum
    # the eval() fake-quant layer's operands, as fp32: the same values, so the same reference and the same bound
    with torch.no_grad():
        xa = llm_qat_amd.mx_quantize(x, "mxfp8_e4m3", rotate=True).float().cpu().double()
        wa = llm_qat_amd.mx_quantize(layer.weight.detach(), "mxfp4", rotate=True).float().cpu().double()
        yq = layer(x).cpu().double()
    ref2, S2 = xa @ wa.T, xa.abs() @ wa.abs().T
    ratio2 = ((out32.cpu().double() - ref2).abs() / (U * S2).clamp_min(1e-300)).max().item()
    print(f"[mx_rot MXLinear tokens={tokens}] against the fake-quant operands' product: {ratio2:.4f}")
    assert ratio2 <= 2 * K
    b = 2 * K * U * S2
    assert ((yq - ref2).abs() <= b + 2.0 ** -9 * (ref2.abs() + b)).all()     # the fake-quant layer itself, rounded once to bf16
    # and against the unrotated float product: the rotated layer computes the same function up to quantization error
    plain = x.float().cpu().double() @ layer.weight.detach().float().cpu().double().T
    print(f"[mx_rot MXLinear tokens={tokens}] relative error to the unquantized product: {((ref - plain).norm() / plain.norm()).item():.4f}")


@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_mx_linear_rotated_compiles_fullgraph(backend):
    if backend == "inductor":
        try:
            import triton  # noqa: F401
        except ImportError:
            pytest.skip("inductor needs triton, which this environment does not have")
    torch._dynamo.reset()
    m, x, _ = linear_case(False)
    mxl = MXLinear.from_quantize_linear(m.eval())
    with torch.no_grad():
        want = mxl(x.detach())
        got = torch.compile(mxl, fullgraph=True, backend=backend)(x.detach())
    assert same_bits(got, want)
