"""The column-block MX quantizer (ops.mx_quantize_axis(axis=-2), fqt_mx_fwd_cols) and QuantizeLinear's MX-quantized backward on the MI355X
(DESIGN.md section 17).  Every comparison is on bit patterns with zero tolerance (any NaN equals any NaN).

The values are checked against the numpy references of the row axis (tests/mx_reference.py: floor, tests/mx_rules_reference.py: ceil),
applied to the transposed bit patterns and transposed back; the shapes come from the kernel's tile, read from csrc/fq_shapes.h."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_reference as M
import mx_rules_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SHAPES_H = open(os.path.join(ROOT, "llm-qat_amd", "csrc", "fq_shapes.h")).read()


def _const(name):
    return int(re.search(rf"^constexpr int {name} = (\d+);", _SHAPES_H, re.M).group(1))


TR, STRIPS = _const("MXC_TILE_ROWS"), _const("MXC_TILE_STRIPS")        # the workgroup's tile: TR rows x STRIPS 16-byte column strips
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}
DTYPES = ["bf16", "fp16", "fp32"]
FMTS = list(M.FORMATS)
RULES = ["floor", "ceil"]


def tile(dtype):
    """-> (V, TC): elements per 16-byte vector, columns of the tile"""
    v = 16 // ESIZE[dtype]
    return v, STRIPS * v


def to_bits(t, dtype):
    return t.detach().contiguous().cpu().view(IDT[dtype]).numpy().view(NDT[dtype])


def from_bits(b, dtype):
    return torch.from_numpy(np.array(b).view(np.int16 if NDT[dtype] is np.uint16 else np.int32)).view(TDT[dtype]).cuda()


def assert_bits_equal(got, want, dtype):
    shape = np.asarray(want).shape
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    gn, wn = np.isnan(M.decode(got, dtype)), np.isnan(M.decode(want, dtype))
    assert np.array_equal(gn, wn), f"NaN positions differ at {[np.unravel_index(i, shape) for i in np.flatnonzero(gn != wn)[:6]]}"
    bad = np.flatnonzero((got != want) & ~wn)
    assert bad.size == 0, f"{bad.size} elements differ, first {[np.unravel_index(i, shape) for i in bad[:4]]}: got {got[bad[:4]]}, want {want[bad[:4]]}"


def assert_same_bits(a, b):
    """two device tensors, bit for bit, any NaN equal to any NaN"""
    assert a.shape == b.shape and a.dtype == b.dtype
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    a, b = a.contiguous(), b.contiguous()
    same = (a.view(it) == b.view(it)) | (a.isnan() & b.isnan())
    assert bool(same.all()), f"{int((~same).sum())} of {a.numel()} elements differ"


def ref_cols(bits, dtype, fmt, rule):
    """the row-axis references on the transposed patterns, transposed back"""
    bt = np.ascontiguousarray(np.swapaxes(bits, -1, -2))
    with np.errstate(over="ignore"):
        y = M.quantize_bits(bt, dtype, fmt) if rule == "floor" else R.quantize_bits(bt, dtype, fmt, "ceil")
    return np.ascontiguousarray(np.swapaxes(y, -1, -2))


@functools.lru_cache(maxsize=None)
def rand_bits(shape, dtype, seed):
    """finite values over many binades (one binade draw per column block, so the blocks differ), with zeros and signed zeros"""
    rng = np.random.default_rng(seed)
    r, c = shape[-2], shape[-1]
    lead = shape[:-2]
    x = rng.standard_normal(shape) * np.exp2(np.repeat(rng.integers(-12, 12, lead + (r // 32, c)), 32, axis=-2).astype(np.float64))
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(4, flat.size // 200))
    flat[idx[::2]] = 0.0
    flat[idx[1::2]] = -0.0
    b = M.encode(x, dtype).reshape(shape)
    b.setflags(write=False)
    return b


def quantize_cols(b, dtype, fmt, rule, counted=True):
    x = from_bits(b, dtype)
    before = dict(ops.mx_counts)
    y = ops.mx_quantize_axis(x, fmt, scale_rule=rule, axis=-2)
    assert y.dtype is TDT[dtype] and y.shape == x.shape and y.is_contiguous()
    if counted:     # the kernel route: one launch of its own, no copy, no row-kernel launch
        assert ops.mx_counts["mx_cols_launch"] == before["mx_cols_launch"] + 1
        assert ops.mx_counts["mx_launch"] == before["mx_launch"] and ops.mx_counts["mx_copy_route"] == before["mx_copy_route"]
    return to_bits(y, dtype)


# ---- against the independent reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_shapes_against_the_reference(dtype, fmt, rule):
    v, tc = tile(dtype)
    seed = 0
    for r in sorted({32, TR, TR + 32, 2 * TR + 32}):
        for c in (v, tc - v, tc, tc + v, 3 * tc + v):
            seed += 1
            b = rand_bits((r, c), dtype, seed)
            assert_bits_equal(quantize_cols(b, dtype, fmt, rule), ref_cols(b, dtype, fmt, rule), dtype)
    b = rand_bits((3, 64, tc + v), dtype, 99)           # a batch of matrices: blocks never straddle two of them
    assert_bits_equal(quantize_cols(b, dtype, fmt, rule), ref_cols(b, dtype, fmt, rule), dtype)


SPECIAL = {   # NaN, +Inf, -Inf, -0.0, smallest subnormal, a larger subnormal, largest finite
    "bf16": (0x7FC1, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x0043, 0x7F7F),
    "fp16": (0x7E01, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x0203, 0x7BFF),
    "fp32": (0x7FC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x00012345, 0x7F7FFFFF),
}


def crafted_bits(dtype):
    """[64, TC + V]: two blocks down every column; the named columns hold one crafted block each, the rest random finite values"""
    v, tc = tile(dtype)
    b = rand_bits((64, tc + v), dtype, 7).copy()
    nan, pinf, ninf, nzero, tiny, sub, big = (NDT[dtype](s) for s in SPECIAL[dtype])
    one, lead = M.encode(np.array([1.0, 1.96875 * 8.0]), dtype)
    b[5, 0] = nan                      # column 0, block 0: one NaN
    b[40, 1] = pinf                    # column 1, block 1
    b[63, 2] = ninf                    # column 2, block 1
    b[0:32, 3] = 0                     # an all-zero block
    b[32:64, 4] = np.where(np.arange(32) % 3 == 0, nzero, 0)     # signed zeros only
    b[0:32, 5] = np.where(np.arange(32) % 2 == 0, tiny, sub)     # subnormal inputs only: amax at the low end of the scale's range
    b[7, 5] |= nzero
    b[32:64, 6] = one                  # the top binade saturates under floor and does not under ceil
    b[33, 6], b[50, 6] = lead, lead | nzero
    b[0:32, 7] = one                   # amax is the dtype's largest finite value: the high end
    b[31, 7] = big
    b[32:64, tc] = 0                   # the same in the last, partial column tile
    b[45, tc] = nan
    b[3, tc + v - 1] = ninf
    return b


@pytest.mark.parametrize("dtype", DTYPES)
def test_crafted_blocks(dtype):
    v, tc = tile(dtype)
    b = crafted_bits(dtype)
    for fmt in FMTS:
        got = {}
        for rule in RULES:
            got[rule] = quantize_cols(b, dtype, fmt, rule)
            want = ref_cols(b, dtype, fmt, rule)
            assert_bits_equal(got[rule], want, dtype)
            y = M.decode(got[rule], dtype)
            nan = np.isnan(y)
            expect = np.zeros_like(nan)
            expect[0:32, 0] = expect[32:64, 1] = expect[32:64, 2] = expect[32:64, tc] = expect[0:32, tc + v - 1] = True
            assert np.array_equal(nan, expect)          # the block is all NaN; its 31 row-neighbours in other columns and the column's other block are not
            assert (got[rule][0:32, 3] == 0).all()
            assert np.array_equal(got[rule][32:64, 4], b[32:64, 4])      # signed zeros keep their signs
        assert M.decode(got["floor"][33:34, 6], dtype)[0] < M.decode(got["ceil"][33:34, 6], dtype)[0] == 16.0      # saturated under floor only
        assert got["floor"][50, 6] != got["ceil"][50, 6]


# ---- against the row kernel -------------------------------------------------------------------------------------------------------------------

def transposed_route(x, fmt, rule):
    return ops.mx_quantize(x.transpose(-1, -2).contiguous(), fmt, scale_rule=rule).transpose(-1, -2).contiguous()


@pytest.mark.parametrize("dtype, shape", [("bf16", (2048, 4096)), ("fp32", (96, 4100)), ("bf16", (4096, 11008))])
def test_equals_the_transposed_route_through_the_row_kernel(dtype, shape):
    """(the last shape is above the library's non-temporal load threshold of 72 MiB: the other load flavour of the kernel)"""
    g = torch.Generator(device="cuda").manual_seed(3)
    x = (torch.randn(shape, device="cuda", generator=g) * torch.exp2(torch.randint(-8, 8, (shape[0] // 32, 1, shape[1]), device="cuda", generator=g)
         .expand(-1, 32, -1).reshape(shape).float())).to(TDT[dtype])
    for fmt, rule in (("mxfp4", "floor"), ("mxfp8_e4m3", "ceil")):
        before = dict(ops.mx_counts)
        y = ops.mx_quantize_axis(x, fmt, scale_rule=rule, axis=-2)
        assert ops.mx_counts["mx_cols_launch"] == before["mx_cols_launch"] + 1 and ops.mx_counts["mx_launch"] == before["mx_launch"]
        assert_same_bits(y, transposed_route(x, fmt, rule))
        del y


# ---- nothing is written outside y ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_canaries_around_y_stay_intact(dtype):
    v, tc = tile(dtype)
    L, guard = _lib.lib(), 4096
    for r, c in ((32, v), (96, tc - v), (32, tc + v), (64, 3 * tc + v)):
        b = rand_bits((r, c), dtype, 11)
        x = from_bits(b, dtype)
        nbytes = r * c * ESIZE[dtype]
        buf = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (buf.data_ptr() + guard) % 16 == 0
        rc = L.fqt_mx_fwd_cols(x.data_ptr(), buf.data_ptr() + guard, r, c, ops.MX_FORMATS["mxfp8_e4m3"], ops._DTYPES[x.dtype], 0, None)
        assert rc == 0, L.fq_last_error()
        torch.cuda.synchronize()
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + nbytes:] == 0xA5).all())
        y = buf[guard:guard + nbytes].view(TDT[dtype]).view(r, c)
        assert_bits_equal(to_bits(y, dtype), ref_cols(b, dtype, "mxfp8_e4m3", "floor"), dtype)


# ---- the other route ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_inputs_the_kernel_does_not_take_go_through_the_row_kernel(dtype):
    v, tc = tile(dtype)
    r, c = 64, tc + v
    b = rand_bits((r, c), dtype, 21)
    x = from_bits(b, dtype)
    flat = torch.empty(r * c + 1, dtype=x.dtype, device="cuda")
    misaligned = flat[1:].view(r, c)
    misaligned.copy_(x)
    wide = torch.empty(r, 2 * c, dtype=x.dtype, device="cuda")
    strided = wide[:, ::2]
    strided.copy_(x)
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 and not strided.is_contiguous()
    bo = rand_bits((r, c + 1), dtype, 22)               # a row that is not whole 16-byte vectors
    for t, bits in ((misaligned, b), (strided, b), (from_bits(bo, dtype), bo)):
        before = dict(ops.mx_counts)
        y = ops.mx_quantize_axis(t, "mxfp6_e3m2", scale_rule="ceil", axis=-2)
        assert y.shape == t.shape and y.is_contiguous()
        assert ops.mx_counts["mx_cols_launch"] == before["mx_cols_launch"]
        assert ops.mx_counts["mx_copy_route"] > before["mx_copy_route"] and ops.mx_counts["mx_launch"] == before["mx_launch"] + 1
        assert_bits_equal(to_bits(y, dtype), ref_cols(bits, dtype, "mxfp6_e3m2", "ceil"), dtype)


# ---- gradient and torch.compile -------------------------------------------------------------------------------------------------------------------

def test_gradient_is_the_incoming_tensor():
    x = from_bits(rand_bits((64, 72), "bf16", 31), "bf16").requires_grad_(True)
    y = llm_qat_amd.mx_quantize_axis(x, "mxfp4", axis=-2)
    assert_same_bits(y.detach(), ops.mx_quantize_axis(x.detach(), "mxfp4", axis=-2))
    g = torch.randn_like(y)
    before = dict(ops.mx_counts)
    y.backward(g)
    assert ops.mx_counts == before                      # no launch backward
    assert_same_bits(x.grad, g)
    (gx,) = torch.autograd.grad(llm_qat_amd.mx_quantize_axis(x, "mxfp4", scale_rule="ceil", axis=0), x, g)      # axis 0 of a matrix is axis -2
    assert_same_bits(gx, g)


def test_traces_under_torch_compile():
    def f(x):
        return llm_qat_amd.mx_quantize_axis(x * 2.0, "mxfp8_e4m3", scale_rule="ceil", axis=-2) + 1.0

    x = from_bits(rand_bits((64, 72), "bf16", 32), "bf16")
    want = f(x)
    got = torch.compile(f, fullgraph=True, backend="aot_eager")(x)
    assert_same_bits(got, want)
    xg = x.clone().requires_grad_(True)
    torch.compile(f, fullgraph=True, backend="aot_eager")(xg).sum().backward()
    assert_same_bits(xg.grad, torch.full_like(x, 2.0))


# ---- QuantizeLinear(mx_backward_format=...) ---------------------------------------------------------------------------------------------------------

IN, OUT = 128, 96
WF, AF = "mxfp4", "mxfp8_e4m3"


def qr(t, fmt, rule):
    return ops.mx_quantize(t, fmt, scale_rule=rule)


def qc_by_rows(t, fmt, rule):
    """the column-axis quantizer obtained through the row-axis API and transposes alone"""
    return qr(t.t().contiguous(), fmt, rule).t().contiguous()


class ReferenceLinear(torch.autograd.Function):
    """DESIGN.md section 17 restated on the row-axis API: the same torch.matmul calls on operands of the same values, shapes and strides"""

    @staticmethod
    def forward(ctx, x, w, rule, fb):
        ctx.save_for_backward(x, w)
        ctx.cfg = (rule, fb)
        return F.linear(qr(x, AF, rule), qr(w, WF, rule))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        rule, fb = ctx.cfg
        with torch.autocast("cuda", enabled=False):
            d = g.dtype
            g2 = g.reshape(-1, OUT).contiguous()
            x2 = x.reshape(-1, IN).to(d)
            gx2 = torch.matmul(qr(g2, fb, rule), qc_by_rows(w.to(d), fb, rule))
            pad = -g2.shape[0] % 32
            if pad:
                g2 = torch.cat([g2, g2.new_zeros(pad, OUT)])
                x2 = torch.cat([x2, x2.new_zeros(pad, IN)])
            gw = torch.matmul(qc_by_rows(g2, fb, rule).t(), qc_by_rows(x2, fb, rule))
        return gx2.reshape(x.shape).to(x.dtype), gw.to(w.dtype), None, None


MODES = {"bf16": (torch.bfloat16, False), "fp32": (torch.float32, False), "autocast": (torch.float32, True)}


def delta(before):
    return {k: v - before[k] for k, v in ops.mx_counts.items() if v != before[k]}


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fb", ["mxfp4", "mxfp8_e4m3"])
@pytest.mark.parametrize("mode", list(MODES))
def test_module_backward_matches_the_reference(mode, fb, rule):
    pdt, autocast = MODES[mode]
    g = torch.Generator(device="cuda").manual_seed(5)
    layer = QuantizeLinear(IN, OUT, w_bits=4, a_bits=8, weight_format=WF, act_format=AF, mx_scale_rule=rule, mx_backward_format=fb).cuda().to(pdt)
    plain = QuantizeLinear(IN, OUT, w_bits=4, a_bits=8, weight_format=WF, act_format=AF, mx_scale_rule=rule).cuda().to(pdt)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(OUT, IN, device="cuda", generator=g) * 0.1)
        plain.weight.copy_(layer.weight)
    for shape in ((64, IN), (40, IN), (2, 20, IN)):
        x = torch.randn(shape, device="cuda", generator=g).to(pdt).requires_grad_(True)
        xr = x.detach().clone().requires_grad_(True)
        wr = layer.weight.detach().clone().requires_grad_(True)
        layer.weight.grad = None
        with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
            before = dict(ops.mx_counts)
            out = layer(x)
            assert delta(before) == {"mx_launch": 2}
            want_out = plain(x.detach())
            ref_out = ReferenceLinear.apply(xr, wr, rule, fb)
        assert out.dtype is (torch.bfloat16 if autocast else pdt)
        assert_same_bits(out.detach(), want_out)
        assert_same_bits(out.detach(), ref_out.detach())
        r = torch.randn(out.shape, device="cuda", generator=g).to(out.dtype)
        tokens = out.numel() // OUT
        before = dict(ops.mx_counts)
        out.backward(r)
        want = {"mx_launch": 1, "mx_cols_launch": 3}
        if tokens % 32:
            want["mx_copy_route"] = 1               # the zero rows that pad the tokens
        assert delta(before) == want
        ref_out.backward(r)
        assert x.grad.dtype is pdt and layer.weight.grad.dtype is pdt
        assert_same_bits(x.grad, xr.grad)
        assert_same_bits(layer.weight.grad, wr.grad)
        assert bool(x.grad.isfinite().all()) and bool(layer.weight.grad.isfinite().all()) and float(layer.weight.grad.abs().max()) > 0


def test_a_gradient_nobody_needs_costs_no_launch():
    layer = QuantizeLinear(IN, OUT, w_bits=4, a_bits=8, weight_format=WF, act_format=AF, mx_backward_format="mxfp8_e4m3").cuda().to(torch.bfloat16)
    x = torch.randn(64, IN, device="cuda", dtype=torch.bfloat16)
    layer.weight.requires_grad_(False)                  # a frozen weight: no Qc(g), no Qc(x)
    out = layer(x.clone().requires_grad_(True))
    before = dict(ops.mx_counts)
    out.backward(torch.ones_like(out))
    assert delta(before) == {"mx_launch": 1, "mx_cols_launch": 1}
    assert layer.weight.grad is None
    layer.weight.requires_grad_(True)                   # an input that needs none: no Qr(g), no Qc(W)
    out = layer(x)
    before = dict(ops.mx_counts)
    out.backward(torch.ones_like(out))
    assert delta(before) == {"mx_cols_launch": 2}
    with torch.no_grad():
        before = dict(ops.mx_counts)
        layer(x)
        assert delta(before) == {"mx_launch": 2}
