"""Scale rule ("floor" / "ceil") and saturation-masked straight-through gradient of the MX quantizer on the MI355X, against the numpy
reference tests/mx_rules_reference.py.  Zero tolerance on bits (any NaN equals any NaN).  The cases come from tests/mx_rules_cases.py;
tests/test_mx_rules_cpu.py proves them sensitive to a wrong mask definition, a wrong scale rule and a wrong backward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import MXLinear, _lib, convert_to_mx_inference, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_rules_reference as R
from mx_reference import decode, pack_fp4
from mx_rules_cases import EXPORT_FMTS, FMTS, exhaustive_bits, grad_bits, rand_bits

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
RULES = ["floor", "ceil"]


def to_bits(t, dtype=None):
    dtype = dtype or NAME[t.dtype]
    return t.detach().contiguous().cpu().view(IDT[dtype]).numpy().view(NDT[dtype])


def from_bits(b, dtype, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16 if NDT[dtype] is np.uint16 else np.int32)).view(TDT[dtype]).to(device)


def assert_bits_equal(got, want, dtype):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    gn, wn = np.isnan(decode(got, dtype)), np.isnan(decode(want, dtype))
    assert np.array_equal(gn, wn), f"NaN positions differ: {np.flatnonzero(gn != wn)[:8]}"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{bad.size} elements differ, first {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}"


def assert_mask_equal(mask, keep):
    assert mask.dtype is torch.uint8 and mask.dim() == 1 and mask.numel() * 8 == keep.size
    got, want = mask.cpu().numpy(), R.pack_mask(keep)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} mask bytes differ, first {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}"


def check_all(b, dtype, fmt, rule, rotate=False):
    """y, the mask, and (FP4 / FP8) the export codes and scale bytes of one tensor against the reference"""
    x = from_bits(b, dtype)
    y, mask = ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=rule, return_mask=True)
    assert y.dtype is TDT[dtype] and y.shape == x.shape
    assert_bits_equal(to_bits(y), R.quantize_bits(b, dtype, fmt, rule, rotate), dtype)
    keep = R.keep_mask(b, dtype, fmt, rule, rotate)
    assert_mask_equal(mask, keep)
    y2 = ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=rule)                 # the same values without the mask
    assert torch.equal(y2.view(IDT[dtype]), y.view(IDT[dtype]))
    if fmt in EXPORT_FMTS:
        e = ops.mx_export(x, fmt, rotate=rotate, scale_rule=rule)
        codes, scales = R.export_bits(b, dtype, fmt, rule, rotate)
        assert np.array_equal(e.scales.cpu().numpy().reshape(-1), scales)
        assert np.array_equal(e.elements.cpu().numpy().reshape(-1), pack_fp4(codes) if fmt == "mxfp4" else codes)
        assert e.rotated is rotate
        assert_bits_equal(to_bits(e.dequantize()), to_bits(y), dtype)
    return keep


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_exhaustive_16bit_values_masks_and_exports(dtype, fmt, rule):
    b = exhaustive_bits(dtype, fmt)
    keep = check_all(b, dtype, fmt, rule)
    v = decode(b, dtype).reshape(-1, 32)
    finite = np.isfinite(v).all(1)
    if rule == "ceil":
        assert keep.all()                                   # no element of a finite block saturates
    else:
        assert not keep.reshape(-1, 32)[finite].all()
    assert keep.reshape(-1, 32)[~finite].all()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_shapes_plain_and_rotated(dtype, fmt, rule):
    for k, shape in enumerate([(3, 32), (257, 96), (2, 3, 4, 64)]):
        check_all(rand_bits(shape, dtype, 10 + k), dtype, fmt, rule)
    for k, shape in enumerate([(3, 64), (130, 192), (2, 3, 4, 128)]):
        check_all(rand_bits(shape, dtype, 20 + k), dtype, fmt, rule, rotate=True)


def test_fp16_rotated_and_saturating_rotated_blocks():
    b = rand_bits((64, 256), "fp16", 31)
    check_all(b, "fp16", "mxfp4", "floor", rotate=True)
    keep = check_all(b, "fp16", "mxfp6_e2m3", "ceil", rotate=True)
    assert keep.all()
    assert not R.keep_mask(b, "fp16", "mxfp4", "floor", True).all()


@pytest.mark.parametrize("shape", [(4096, 11008), (4097, 96), (2, 3, 8, 64)])
def test_ex_entry_points_reproduce_the_existing_ones(shape):
    """flags 0 is fq_mx_fwd / fq_mx_export byte for byte, FQ_MX_FLAG_ROTATE the *_rot entry points (cols % 64 == 0 only)"""
    L = _lib.lib()
    for dtype, fmt in (("bf16", "mxfp4"), ("fp32", "mxfp8_e4m3")) if shape[0] != 4096 else (("bf16", "mxfp4"),):
        x = from_bits(rand_bits(shape, dtype, 40), dtype)
        cols = shape[-1]
        rows = x.numel() // cols
        code, dt = ops.MX_FORMATS[fmt], ops._DTYPES[x.dtype]
        for rot in ([False, True] if cols % 64 == 0 else [False]):
            flags = _lib.MX_FLAG_ROTATE if rot else 0
            y_old, y_new, y_m = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device="cuda")
            assert (L.fq_mx_fwd_rot if rot else L.fq_mx_fwd)(x.data_ptr(), y_old.data_ptr(), rows, cols, code, dt, None) == 0
            assert L.fq_mx_fwd_ex(x.data_ptr(), y_new.data_ptr(), None, rows, cols, code, dt, flags, None) == 0
            assert L.fq_mx_fwd_ex(x.data_ptr(), y_m.data_ptr(), mask.data_ptr(), rows, cols, code, dt, flags, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(y_old.view(torch.uint8), y_new.view(torch.uint8)) and torch.equal(y_old.view(torch.uint8), y_m.view(torch.uint8))
            nel = x.numel() // (2 if fmt == "mxfp4" else 1)
            outs = [(torch.empty(nel, dtype=torch.uint8, device="cuda"), torch.empty(x.numel() // 32, dtype=torch.uint8, device="cuda")) for _ in range(2)]
            assert (L.fq_mx_export_rot if rot else L.fq_mx_export)(x.data_ptr(), outs[0][0].data_ptr(), outs[0][1].data_ptr(), rows, cols, code, dt, None) == 0
            assert L.fq_mx_export_ex(x.data_ptr(), outs[1][0].data_ptr(), outs[1][1].data_ptr(), rows, cols, code, dt, flags, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            # and the Python defaults are today's calls
            assert torch.equal(ops.mx_quantize(x, fmt, rotate=rot).view(torch.uint8), y_old.view(torch.uint8))


def saturating_bits(shape, dtype, seed):
    """random blocks, every third led by a value whose top binade saturates under floor for every format (mantissa 1.96875)"""
    b = rand_bits(shape, dtype, seed)
    blk = b.reshape(-1, 32)
    lead = R.encode(np.array([1.96875 * 2.0 ** 3, -1.96875 * 2.0 ** 3, 1.0]), dtype)
    blk[::3, :] = lead[2]
    blk[::3, 0], blk[::3, 7], blk[::3, 20] = lead[0], lead[1], lead[0]
    return b


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_backward_is_exact(dtype, rotate):
    # (rotated: the leaders of saturating_bits are spread over their run, and what saturates is the top of each rotated block -- about one
    # element in a hundred, so the rotated shapes are larger)
    for k, shape in enumerate([(64, 64), (257, 192), (2, 3, 16, 128)] if rotate else [(4, 64), (257, 192), (2, 3, 4, 128)]):
        b = saturating_bits(shape, dtype, 50 + k)
        keep = R.keep_mask(b, dtype, "mxfp4", "floor", rotate)
        assert 0 < (~keep).sum() < keep.size
        _, mask = ops.mx_quantize(from_bits(b, dtype), "mxfp4", rotate=rotate, return_mask=True)
        assert_mask_equal(mask, keep)
        gb = grad_bits(keep, dtype, 60 + k)
        gv = decode(gb, dtype)
        assert np.isnan(gv[~keep]).any() and np.isinf(gv[~keep]).any() and np.isnan(gv[keep]).any() and np.isinf(gv[keep]).any()
        g = from_bits(gb, dtype)
        llm_qat_amd.stats(reset=True)
        gx = ops.mx_ste_backward(g, mask, rotate=rotate)
        st = llm_qat_amd.stats()
        assert st.get("mx_ste_launch") == 1 and not st.get("mx_rotate_launch") and not st.get("mx_launch")       # one launch, rotated or not
        assert gx.shape == g.shape and gx.dtype is g.dtype
        want = R.ste_backward_bits(gb, keep, dtype, rotate)
        if rotate:
            assert_bits_equal(to_bits(gx), want, dtype)
            masked = from_bits(R.ste_backward_bits(gb, keep, dtype, False), dtype)                               # = fq_block_rotate of the masked g
            assert_bits_equal(to_bits(gx), to_bits(ops.mx_rotate(masked)), dtype)      # (two NaN operands of an add: either payload)
        else:
            assert np.array_equal(to_bits(gx), want)            # a select: NaN payloads and -0.0 kept bit for bit, +0.0 at the masked ones


def test_backward_in_place_without_rotation_and_refused_with_it():
    L = _lib.lib()
    b = saturating_bits((64, 128), "bf16", 70)
    x = from_bits(b, "bf16")
    _, mask = ops.mx_quantize(x, "mxfp4", return_mask=True)
    keep = R.keep_mask(b, "bf16", "mxfp4")
    gb = grad_bits(keep, "bf16", 71)
    g = from_bits(gb, "bf16")
    dt = ops._DTYPES[g.dtype]
    assert L.fq_mx_ste_bwd(g.data_ptr(), mask.data_ptr(), g.data_ptr(), 64, 128, dt, 0, None) == 0            # gx == g
    torch.cuda.synchronize()
    assert np.array_equal(to_bits(g), R.ste_backward_bits(gb, keep, "bf16"))
    assert L.fq_mx_ste_bwd(g.data_ptr(), mask.data_ptr(), g.data_ptr(), 64, 128, dt, _lib.MX_FLAG_ROTATE, None) == -7


def test_canaries_around_y_mask_and_gx():
    L = _lib.lib()
    for dtype, fmt, rot in (("bf16", "mxfp4", False), ("fp32", "mxfp8_e5m2", False), ("fp16", "mxfp6_e2m3", True), ("fp32", "mxfp4", True)):
        rows, cols = 37, 192
        b = saturating_bits((rows, cols), dtype, 80)
        x = from_bits(b, dtype)
        es, n, pad = x.element_size(), rows * cols, 256
        flags = (_lib.MX_FLAG_ROTATE if rot else 0)
        ybuf = torch.full((n * es + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
        mbuf = torch.full((n // 8 + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda")
        gxbuf = torch.full((n * es + 2 * pad,), 0x3C, dtype=torch.uint8, device="cuda")
        code, dt = ops.MX_FORMATS[fmt], ops._DTYPES[x.dtype]
        assert L.fq_mx_fwd_ex(x.data_ptr(), ybuf.data_ptr() + pad, mbuf.data_ptr() + pad, rows, cols, code, dt, flags, None) == 0
        keep = R.keep_mask(b, dtype, fmt, "floor", rot)
        gb = grad_bits(keep, dtype, 81)
        g = from_bits(gb, dtype)
        assert L.fq_mx_ste_bwd(g.data_ptr(), mbuf.data_ptr() + pad, gxbuf.data_ptr() + pad, rows, cols, dt, flags, None) == 0
        torch.cuda.synchronize()
        for buf, val, nb in ((ybuf, 0xA5, n * es), (mbuf, 0x5A, n // 8), (gxbuf, 0x3C, n * es)):
            assert (buf[:pad] == val).all() and (buf[pad + nb:] == val).all()
        assert_bits_equal(to_bits(ybuf[pad: pad + n * es].view(x.dtype)), R.quantize_bits(b, dtype, fmt, "floor", rot), dtype)
        assert_mask_equal(mbuf[pad: pad + n // 8].clone(), keep)
        assert_bits_equal(to_bits(gxbuf[pad: pad + n * es].view(x.dtype)), R.ste_backward_bits(gb, keep, dtype, rot), dtype)


def test_misaligned_and_transposed_inputs_take_one_copy():
    x = (torch.randn(64 * 128 + 8, device="cuda") * 3).bfloat16()
    v = x.view(-1)[1:1 + 64 * 128].view(64, 128)          # 2-byte offset: not 16-byte aligned
    assert v.data_ptr() % 16
    llm_qat_amd.stats(reset=True)
    y, mask = ops.mx_quantize(v, "mxfp4", scale_rule="ceil", return_mask=True)
    st = llm_qat_amd.stats()
    assert st.get("mx_copy_route") == 1 and st.get("mx_launch") == 1 and st.get("mx_mask_launch") == 1
    assert_bits_equal(to_bits(y), R.quantize_bits(to_bits(v), "bf16", "mxfp4", "ceil"), "bf16")
    w = torch.randn(128, 96, device="cuda").half() * 5
    wt = w.t()                                             # [96, 128], transposed
    llm_qat_amd.stats(reset=True)
    y, mask = ops.mx_quantize(wt, "mxfp4", rotate=True, return_mask=True)
    assert llm_qat_amd.stats().get("mx_copy_route") == 1
    keep = R.keep_mask(to_bits(wt), "fp16", "mxfp4", "floor", True)
    assert_mask_equal(mask, keep)
    e = ops.mx_export(wt, "mxfp8_e4m3", scale_rule="ceil")
    assert np.array_equal(e.scales.cpu().numpy().reshape(-1), R.export_bits(to_bits(wt), "fp16", "mxfp8_e4m3", "ceil")[1])
    g = torch.randn(128, 96, device="cuda").half().t()     # a transposed gradient
    llm_qat_amd.stats(reset=True)
    gx = ops.mx_ste_backward(g, mask, rotate=True)
    st = llm_qat_amd.stats()
    assert st.get("mx_copy_route") == 1 and st.get("mx_ste_launch") == 1
    assert_bits_equal(to_bits(gx), R.ste_backward_bits(to_bits(g), keep, "fp16", True), "fp16")
    big = torch.zeros(mask.numel() + 16, dtype=torch.uint8, device="cuda")
    big[1:1 + mask.numel()] = mask                          # a misaligned mask
    llm_qat_amd.stats(reset=True)
    gx2 = ops.mx_ste_backward(g.contiguous(), big[1:1 + mask.numel()], rotate=True)
    assert llm_qat_amd.stats().get("mx_copy_route") == 1 and torch.equal(gx2.view(torch.int16), gx.view(torch.int16))


# ---- QuantizeLinear: output and both gradients against F.linear of reference-quantized operands with reference-masked gradients -------

def ref_q(t, fmt, rule, rotate):
    dtype = NAME[t.dtype]
    return from_bits(R.quantize_bits(to_bits(t), dtype, fmt, rule, rotate).reshape(tuple(t.shape)), dtype, t.device)


def ref_bwd(g, t, fmt, rule, rotate):
    """the masked gradient of the quantizer of t, by the reference, in g's dtype"""
    keep = R.keep_mask(to_bits(t), NAME[t.dtype], fmt, rule, rotate)
    dtype = NAME[g.dtype]
    return from_bits(R.ste_backward_bits(to_bits(g), keep, dtype, rotate).reshape(tuple(g.shape)), dtype, g.device)


CONFIGS = {"plain": {}, "rotate": {"mx_rotate": True}, "ceil": {"mx_scale_rule": "ceil"}}


def linear_case(master_fp32, **kw):
    torch.manual_seed(5)
    m = QuantizeLinear(256, 192, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_ste="clip", **kw).cuda()
    with torch.no_grad():
        m.weight.mul_(3)
        m.weight.view(-1, 32)[::7, 5] = 0.234375        # 1.875 * 2^-3 above the uniform init's bound 0.1875: t = 7.5 saturates in E2M1 under floor
    if not master_fp32:
        m = m.bfloat16()
    x = (torch.randn(2, 64, 256, device="cuda") * 2).bfloat16()
    x.view(-1, 32)[::5, 3] = 15.5                       # mantissa 1.9375: the top binade of these blocks saturates under floor (E4M3 and E2M1)
    x.requires_grad_(True)
    g = torch.randn(2, 64, 192, device="cuda").bfloat16()
    return m, x, g


def reference_step(m, x, g, autocast):
    w = m.weight.detach().clone().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    rule, rot = m.mx_scale_rule, m.mx_rotate

    class STE(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, fmt):
            ctx.t, ctx.fmt = t.detach(), fmt
            return ref_q(t, fmt, rule, rot)

        @staticmethod
        def backward(ctx, go):
            return ref_bwd(go, ctx.t, ctx.fmt, rule, rot), None
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
        assert_bits_equal(to_bits(u), to_bits(v), NAME[u.dtype])


@pytest.mark.parametrize("master_fp32", [False, True])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_quantize_linear_clip_matches_reference(config, master_fp32):
    m, x, g = linear_case(master_fp32, **CONFIGS[config])
    if config != "ceil":     # the case does exercise the mask
        for t, fmt in ((x, "mxfp8_e4m3"), (m.weight, "mxfp4")):
            assert not R.keep_mask(to_bits(t), NAME[t.dtype], fmt, "floor", m.mx_rotate).all()
    saved = []
    llm_qat_amd.stats(reset=True)
    xx = x.detach().clone().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        with torch.autocast("cuda", torch.bfloat16, enabled=master_fp32):
            q = llm_qat_amd.mx_quantize(xx, "mxfp8_e4m3", rotate=m.mx_rotate, scale_rule=m.mx_scale_rule, ste="clip")
    assert [(t.dtype, t.numel()) for t in saved] == [(torch.uint8, x.numel() // 8)]         # the bitmap only
    del q
    llm_qat_amd.stats(reset=True)
    with torch.autocast("cuda", torch.bfloat16, enabled=master_fp32):
        out = m(xx)
    st = llm_qat_amd.stats(reset=True)
    assert st.get("mx_launch") == 2 and st.get("mx_mask_launch") == 2 and not st.get("pair_launch") and not st.get("cpp_pair_forward")
    out.backward(g)
    st = llm_qat_amd.stats()
    assert st.get("mx_ste_launch") == 2 and not st.get("mx_launch") and not st.get("mx_rotate_launch")     # one launch per operand gradient
    assert_same((out.detach(), xx.grad, m.weight.grad), reference_step(m, x, g, master_fp32))


def test_identity_ste_under_ceil_saves_nothing_and_launches_no_backward():
    x = (torch.randn(8, 256, device="cuda") * 4).bfloat16().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = llm_qat_amd.mx_quantize(x, "mxfp4", scale_rule="ceil")
    assert saved == []
    assert_bits_equal(to_bits(y), R.quantize_bits(to_bits(x), "bf16", "mxfp4", "ceil"), "bf16")
    g = torch.randn_like(y)
    llm_qat_amd.stats(reset=True)
    (gx,) = torch.autograd.grad(y, x, g)
    assert torch.equal(gx.view(torch.int16), g.view(torch.int16))
    st = llm_qat_amd.stats()
    assert not st.get("mx_launch") and not st.get("mx_ste_launch")


@pytest.mark.parametrize("config", list(CONFIGS))
def test_quantize_linear_clip_checkpointing(config):
    from torch.utils.checkpoint import checkpoint
    m, x, g = linear_case(False, **CONFIGS[config])
    got = module_step(m, x, g, False, fn=lambda t: checkpoint(m, t, use_reentrant=False))
    assert_same(got, reference_step(m, x, g, False))


@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
@pytest.mark.parametrize("config", list(CONFIGS) + ["ceil_identity"])
def test_quantize_linear_compiled(config, backend):
    if backend == "inductor":
        try:
            import triton  # noqa: F401
        except ImportError:
            pytest.skip("inductor needs triton, which this environment does not have")
    torch._dynamo.reset()
    if config == "ceil_identity":
        m, x, g = linear_case(False, mx_scale_rule="ceil")
        m.mx_ste = "identity"
    else:
        m, x, g = linear_case(False, **CONFIGS[config])
    cm = torch.compile(m, fullgraph=True, backend=backend)
    llm_qat_amd.stats(reset=True)
    got = module_step(m, x, g, False, fn=cm)
    st = llm_qat_amd.stats()
    if config != "ceil_identity":
        assert st.get("mx_mask_launch") == 2 and st.get("mx_ste_launch") == 2 and not st.get("mx_rotate_launch")
    assert_same(got, reference_step(m, x, g, False) if config != "ceil_identity" else module_step(m, x, g, False))


def test_create_graph_through_the_masked_backward():
    m, x, g = linear_case(False)
    xx = x.detach().clone().requires_grad_(True)
    y = llm_qat_amd.mx_quantize(xx, "mxfp4", ste="clip")
    go = torch.randn_like(y).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, xx, go, create_graph=True)
    keep = torch.from_numpy(R.keep_mask(to_bits(xx), "bf16", "mxfp4")).cuda()
    assert torch.equal(gx, torch.where(keep, go, torch.zeros_like(go)))
    (ggo,) = torch.autograd.grad(gx.float().sum(), go)
    assert torch.equal(ggo, keep.to(go.dtype))


# ---- inference: ceil exports on the block-scaled GEMM ------------------------------------------------------------------------------------

def _integer_operand(rows, K, seed):
    """small integers times a per-block power of two: every value, every quantized value under either rule and every partial sum of a
    product of two such operands is an integer far below 2^24, so any summation order gives the same fp32 bits"""
    rng = np.random.default_rng(seed)
    v = rng.choice(np.array([0, 1, 2, 3, 4, 6, 7, -1, -2, -3, -5, -7], dtype=np.float64), size=(rows, K))
    v.reshape(-1, 32)[:, 0] = 7.0                                   # amax 7 * 2^s: floor saturates it in FP4, ceil takes E + 1
    s = rng.integers(0, 3, size=(rows, K // 32))
    return torch.from_numpy(v * np.exp2(np.repeat(s, 32, axis=1))).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("a_fmt,w_fmt", [("mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp4"), ("mxfp8_e5m2", "mxfp8_e4m3")])
@pytest.mark.parametrize("M", [8, 160])
def test_ceil_exports_are_exact_on_the_gemm(M, a_fmt, w_fmt):
    K, N = 256, 96
    a, w = _integer_operand(M, K, 1), _integer_operand(N, K, 2)
    ea, ew = ops.mx_export(a, a_fmt, scale_rule="ceil"), ops.mx_export(w, w_fmt, scale_rule="ceil")
    for t, e, fmt in ((a, ea, a_fmt), (w, ew, w_fmt)):
        codes, scales = R.export_bits(to_bits(t), "bf16", fmt, "ceil")
        assert np.array_equal(e.scales.cpu().numpy().reshape(-1), scales)
        assert np.array_equal(e.elements.cpu().numpy().reshape(-1), pack_fp4(codes) if fmt == "mxfp4" else codes)
        if fmt == "mxfp4":
            assert not torch.equal(e.scales, ops.mx_export(t, fmt).scales)         # the rule is in effect
    da, dw = ea.dequantize().double(), ew.dequantize().double()
    ref = da @ dw.t()
    assert ref.abs().max() < 2 ** 24 and torch.equal(ref, ref.round())
    out = ops.mx_matmul(ea, ew, out_dtype=torch.float32)
    assert torch.equal(out.double(), ref)


def test_mx_linear_ceil_equals_export_and_matmul_by_hand_and_the_converter_carries_the_rule():
    torch.manual_seed(3)
    q = QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_scale_rule="ceil").cuda().bfloat16()
    with torch.no_grad():
        q.weight.mul_(3)
    x = (torch.randn(40, 256, device="cuda") * 2).bfloat16()
    ew = q.export_weight()
    codes, scales = R.export_bits(to_bits(q.weight), "bf16", "mxfp4", "ceil")
    assert np.array_equal(ew.scales.cpu().numpy().reshape(-1), scales) and np.array_equal(ew.elements.cpu().numpy().reshape(-1), pack_fp4(codes))
    m = MXLinear.from_quantize_linear(q)
    assert m.scale_rule == "ceil" and torch.equal(m.weight_elements, ew.elements) and torch.equal(m.weight_scales, ew.scales)
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        y = m(x)
    st = llm_qat_amd.stats()
    assert st.get("mx_export_launch") == 1 and st.get("mx_gemm_launch") == 1
    want = ops.mx_matmul(ops.mx_export(x, "mxfp8_e4m3", scale_rule="ceil"), ew, out_dtype=torch.bfloat16)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    floor = ops.mx_matmul(ops.mx_export(x, "mxfp8_e4m3"), ew, out_dtype=torch.bfloat16)
    assert not torch.equal(y.view(torch.int16), floor.view(torch.int16))            # the activation's rule matters
    hand = MXLinear(256, 64, scale_rule="ceil").cuda()
    hand.weight_elements.copy_(ew.elements)
    hand.weight_scales.copy_(ew.scales)
    with torch.no_grad():
        assert torch.equal(hand(x).view(torch.int16), y.view(torch.int16))
    model = torch.nn.Sequential(q, torch.nn.ReLU())
    assert convert_to_mx_inference(model) == 1 and isinstance(model[0], MXLinear) and model[0].scale_rule == "ceil"
    torch._dynamo.reset()
    cm = torch.compile(m, fullgraph=True, backend="aot_eager")
    with torch.no_grad():
        assert torch.equal(cm(x).view(torch.int16), y.view(torch.int16))


def test_process_defaults_reach_unchanged_model_code():
    prev = llm_qat_amd.default_mx_formats(weight="mxfp4", act="mxfp8_e4m3")
    r, s = llm_qat_amd.default_mx_scale_rule("ceil"), llm_qat_amd.default_mx_ste("clip")
    try:
        m = QuantizeLinear(256, 192, bias=False, w_bits=4, a_bits=8).cuda().bfloat16()   # the reference's constructor call
    finally:
        llm_qat_amd.default_mx_formats(*prev)
        llm_qat_amd.default_mx_scale_rule(r)
        llm_qat_amd.default_mx_ste(s)
    x = torch.randn(4, 256, device="cuda").bfloat16()
    llm_qat_amd.stats(reset=True)
    out = m(x)
    assert llm_qat_amd.stats().get("mx_launch") == 2
    assert torch.equal(out, F.linear(ref_q(x, "mxfp8_e4m3", "ceil", False), ref_q(m.weight.detach(), "mxfp4", "ceil", False)))
