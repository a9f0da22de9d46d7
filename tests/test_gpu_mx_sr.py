"""MX fake quantization with stochastic rounding on the MI355X: ops.mx_quantize_sr along both axes (fqs_mx_fwd,
fqs_mx_fwd_cols), the public function and QuantizeLinear(mx_backward_rounding="stochastic").  Every comparison is on bit patterns with
zero tolerance (any NaN equals any NaN).

The values are checked against tests/mx_sr_reference.py (its own Philox4x32-10, the rule restated on the float64 grid); the shapes come from
the kernels' launch constants, read from csrc/fq_launch.h and csrc/fq_shapes.h.

The noise index beyond 2^35.  A tensor whose flat index crosses 2^35 is 64 GiB of bf16 in and 64 GiB out per launch; the suite shares its
device, so no test allocates that.  The 64-bit counter path is tested through fqs_mx_noise, the host function that runs the kernels' own
index-to-word code, in tests/test_mx_sr_cpu.py (indices up to 2^63), and here the device is checked to draw the words that function names."""
import ctypes
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
import mx_sr_reference as S
import test_gpu_mx_cols as parent

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "llm-qat_amd", "csrc")
_SHAPES_H = open(os.path.join(_CSRC, "fq_shapes.h")).read()
_LAUNCH_H = open(os.path.join(_CSRC, "fq_launch.h")).read()


def _const(name):
    return int(re.search(rf"^constexpr int {name} = (\d+);", _SHAPES_H, re.M).group(1))


TR, STRIPS = _const("MXC_TILE_ROWS"), _const("MXC_TILE_STRIPS")        # the column kernel's tile: TR rows x STRIPS 16-byte column strips
_m = re.search(r"constexpr int MX_TPB = (\d+), MX_VPT = (\d+);", _LAUNCH_H)
WG_VECS = int(_m.group(1)) * int(_m.group(2))                          # 16-byte vectors of one workgroup of the row kernel
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}
DTYPES = ["bf16", "fp16", "fp32"]
FMTS = list(M.FORMATS)
RULES = ["floor", "ceil"]
U64 = 2 ** 64 - 1
KEYS = [(0, 0), (U64, U64), (0x9A3C51D20B7E44F1, 0x1F00000003)]        # both 32-bit halves of the key and of the stream words


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


@functools.lru_cache(maxsize=None)
def rand_bits(shape, dtype, seed, axis=-1):
    """finite values over many binades (one binade draw per block along `axis`), with zeros and signed zeros"""
    rng = np.random.default_rng(seed)
    if axis == -1:
        scale = np.repeat(rng.integers(-12, 12, shape[:-1] + (shape[-1] // 32,)), 32, axis=-1)
    else:
        scale = np.repeat(rng.integers(-12, 12, shape[:-2] + (shape[-2] // 32, shape[-1])), 32, axis=-2)
    x = rng.standard_normal(shape) * np.exp2(scale.astype(np.float64))
    flat = x.reshape(-1)
    idx = rng.integers(0, flat.size, max(4, flat.size // 200))
    flat[idx[::2]] = 0.0
    flat[idx[1::2]] = -0.0
    b = M.encode(x, dtype).reshape(shape)
    b.setflags(write=False)
    return b


def delta(before):
    return {k: v - before[k] for k, v in ops.mx_counts.items() if v != before[k]}


def quantize(b, dtype, fmt, rule, seed, stream, axis=-1):
    """one launch of its own kernel, no copy -> the output's bit patterns"""
    x = from_bits(b, dtype)
    before = dict(ops.mx_counts)
    y = ops.mx_quantize_sr(x, fmt, seed, stream, rule, axis)
    assert y.dtype is TDT[dtype] and y.shape == x.shape and y.is_contiguous()
    assert delta(before) == {"mx_sr_launch" if axis == -1 else "mx_sr_cols_launch": 1}
    return to_bits(y, dtype)


# ---- against the independent reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_kernel_against_the_reference(dtype, fmt, rule):
    """flat tensors of whole blocks (a block is bv vectors: the smallest step) one block short of, exactly, and one block past a workgroup's
    vectors, and three workgroups plus a block; every (seed, stream) pair at every size"""
    epv = 16 // ESIZE[dtype]
    bv = 32 // epv
    for k, vecs in enumerate((WG_VECS - bv, WG_VECS, WG_VECS + bv, 3 * WG_VECS + bv)):
        b = rand_bits((vecs * epv,), dtype, 100 + k)
        for seed, stream in KEYS:
            assert_bits_equal(quantize(b, dtype, fmt, rule, seed, stream), S.quantize_bits(b, dtype, fmt, rule, seed, stream), dtype)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_kernel_against_the_reference(dtype, fmt, rule):
    """the reference with column blocks and the flat indices r * cols + c"""
    v = 16 // ESIZE[dtype]
    tc = STRIPS * v
    k = 0
    for r in (32, 64, 96):
        for c in (v, tc - v, tc, tc + v, 3 * tc + v):
            seed, stream = KEYS[k % 3]
            k += 1
            b = rand_bits((r, c), dtype, 200 + k, -2)
            assert_bits_equal(quantize(b, dtype, fmt, rule, seed, stream, -2), S.quantize_bits(b, dtype, fmt, rule, seed, stream, -2), dtype)
    b = rand_bits((3, 64, tc + v), dtype, 299, -2)          # a batch of matrices: blocks never straddle two of them, the index runs through
    seed, stream = KEYS[2]
    assert_bits_equal(quantize(b, dtype, fmt, rule, seed, stream, -2), S.quantize_bits(b, dtype, fmt, rule, seed, stream, -2), dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_both_kernels_index_the_noise_the_same_way(dtype):
    """a tensor whose every element sits at the midpoint of its two neighbours goes up exactly where R16 < 32768: the pattern of ups is the
    noise itself, the same for both axes, and the one fqs_mx_noise names for those flat indices"""
    v = 16 // ESIZE[dtype]
    r, c = 64, STRIPS * v + 32
    x = torch.full((r, c), 2.5, dtype=TDT[dtype], device="cuda")       # mxfp4, amax 2.5: E = -1, the grid around 2.5 is 2 and 3
    seed, stream = KEYS[2]
    rows = ops.mx_quantize_sr(x, "mxfp4", seed, stream)
    cols = ops.mx_quantize_sr(x, "mxfp4", seed, stream, axis=-2)
    assert_same_bits(rows, cols)
    out = (ctypes.c_uint16 * (r * c))()
    assert _lib.lib().fqs_mx_noise(seed, stream, 0, r * c, ops._DTYPES[x.dtype], out) == 0
    up = torch.from_numpy((np.array(out[:], dtype=np.uint16) < 32768).reshape(r, c)).cuda()
    assert bool((rows == torch.where(up, 3.0, 2.0).to(x.dtype)).all()) and 0.4 < float(up.float().mean()) < 0.6


SPECIAL = {   # NaN, +Inf, -Inf, -0.0, smallest subnormal, a larger subnormal, largest finite
    "bf16": (0x7FC1, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x0043, 0x7F7F),
    "fp16": (0x7E01, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x0203, 0x7BFF),
    "fp32": (0x7FC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x00012345, 0x7F7FFFFF),
}


def crafted_bits(dtype):
    """[16, 256], the blocks along the last axis (the column test transposes it): the named rows hold one crafted block each, the rest random
    finite values"""
    b = rand_bits((16, 256), dtype, 7).copy()
    nan, pinf, ninf, nzero, tiny, sub, big = (NDT[dtype](s) for s in SPECIAL[dtype])
    one, lead = M.encode(np.array([1.0, 1.96875 * 8.0]), dtype)
    b[0, 5] = nan                                  # row 0, block 0: one NaN
    b[1, 40] = pinf                                # row 1, block 1
    b[2, 63] = ninf                                # row 2, block 1
    b[3, 0:32] = 0                                 # an all-zero block
    b[4, 32:64] = np.where(np.arange(32) % 3 == 0, nzero, 0)     # signed zeros only
    b[5, 0:32] = np.where(np.arange(32) % 2 == 0, tiny, sub)     # subnormal inputs only
    b[5, 7] |= nzero
    b[6, 32:64] = one                              # the top binade saturates under floor and does not under ceil
    b[6, 33], b[6, 50] = lead, lead | nzero
    b[7, 0:32] = one                               # amax is the dtype's largest finite value
    b[7, 31] = big
    return b


@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_crafted_blocks(dtype, axis):
    b = crafted_bits(dtype)
    if axis == -2:                                 # the same blocks, running down the columns of a [256, 16] tensor
        b = np.ascontiguousarray(b.T)
    at = (lambda r, c: (r, c)) if axis == -1 else (lambda r, c: (c, r))
    seed, stream = KEYS[2]
    for fmt in FMTS:
        got = {}
        for rule in RULES:
            got[rule] = quantize(b, dtype, fmt, rule, seed, stream, axis)
            assert_bits_equal(got[rule], S.quantize_bits(b, dtype, fmt, rule, seed, stream, axis), dtype)
            g = got[rule] if axis == -1 else got[rule].T
            nan = np.isnan(M.decode(g, dtype))
            expect = np.zeros_like(nan)
            expect[0, 0:32] = expect[1, 32:64] = expect[2, 32:64] = True
            assert np.array_equal(nan, expect)      # the block is all NaN and no other is
            assert (g[3, 0:32] == 0).all()
            assert np.array_equal(g[4, 32:64], (b if axis == -1 else b.T)[4, 32:64])      # signed zeros keep their signs
        pf, pc = (S.parts(b, dtype, fmt, rule, seed, stream, axis) for rule in RULES)
        for pos, sign in ((at(6, 33), 1.0), (at(6, 50), -1.0)):     # 15.75 in a block of ones: saturated under floor only
            assert pf["lo"][pos] == pf["hi"][pos] < 15.75 and M.decode(got["floor"][pos].reshape(1), dtype)[0] == sign * pf["hi"][pos]
            assert pc["lo"][pos] < 15.75 < pc["hi"][pos] and abs(M.decode(got["ceil"][pos].reshape(1), dtype)[0]) in (pc["lo"][pos], pc["hi"][pos])


@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_grid_points_stay_and_midpoints_go_up_as_often_as_the_reference_says(dtype, axis):
    """2^16 positions each: an element exactly on a grid point (every seed leaves it), one exactly at a midpoint (f = 1 / 2: up iff
    R16 < 32768 -- the count of ups equals the reference's exactly, and is near half)"""
    n = 1 << 16
    shape = (n // 32, 64) if axis == -1 else (64, n // 32)
    x = np.zeros(shape)
    blk = np.full(32, 1.0)
    blk[0], blk[1] = 6.0, 2.5                       # mxfp4, amax 6: E = 0; 1.0 is on the grid, 2.5 is the midpoint of 2 and 3
    blk[2:] = np.where(np.arange(30) % 2 == 0, 1.0, 2.5)
    if axis == -1:
        x[:, :32] = blk
        x[:, 32:] = blk[::-1]
    else:
        x[:32, :] = blk[:, None]
        x[32:, :] = blk[::-1, None]
    b = M.encode(x, dtype)
    for seed, stream in KEYS[1:]:
        got = quantize(b, dtype, "mxfp4", "floor", seed, stream, axis)
        y = M.decode(got, dtype)
        p = S.parts(b, dtype, "mxfp4", "floor", seed, stream, axis)
        assert (y[x == 1.0] == 1.0).all() and (y[x == 6.0] == 6.0).all()
        mid = x == 2.5
        assert mid.sum() == n and set(np.unique(y[mid])) == {2.0, 3.0}
        assert int((y[mid] == 3.0).sum()) == int(p["up"][mid].sum())
        assert abs(int((y[mid] == 3.0).sum()) - n // 2) < 6 * np.sqrt(n) / 2
        assert_bits_equal(got, M.encode(p["y"], dtype), dtype)


# ---- memory and routing ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_canaries_around_y_stay_intact(dtype):
    v = 16 // ESIZE[dtype]
    tc = STRIPS * v
    L, guard = _lib.lib(), 4096
    cases = [("fqs_mx_fwd_cols", -2, 32, v), ("fqs_mx_fwd_cols", -2, 96, tc - v), ("fqs_mx_fwd_cols", -2, 64, 3 * tc + v),
             ("fqs_mx_fwd", -1, 1, (WG_VECS - 32 // v) * v), ("fqs_mx_fwd", -1, 3, 32), ("fqs_mx_fwd", -1, 1, (WG_VECS + 32 // v) * v)]
    for name, axis, r, c in cases:
        b = rand_bits((r, c), dtype, 11, axis)
        x = from_bits(b, dtype)
        nbytes = r * c * ESIZE[dtype]
        buf = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (buf.data_ptr() + guard) % 16 == 0
        rc = getattr(L, name)(x.data_ptr(), buf.data_ptr() + guard, r, c, ops.MX_FORMATS["mxfp8_e4m3"], ops._DTYPES[x.dtype], 0, 5, 6, None)
        assert rc == 0, L.fq_last_error()
        torch.cuda.synchronize()
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + nbytes:] == 0xA5).all())
        y = buf[guard:guard + nbytes].view(TDT[dtype]).view(r, c)
        assert_bits_equal(to_bits(y, dtype), S.quantize_bits(b, dtype, "mxfp8_e4m3", "floor", 5, 6, axis), dtype)


@pytest.mark.parametrize("axis", [-1, -2])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_non_contiguous_and_misaligned_inputs_give_the_contiguous_bits(dtype, axis):
    v = 16 // ESIZE[dtype]
    r, c = 64, STRIPS * v + 32
    b = rand_bits((r, c), dtype, 21, axis)
    x = from_bits(b, dtype)
    flat = torch.empty(r * c + 1, dtype=x.dtype, device="cuda")
    misaligned = flat[1:].view(r, c)
    misaligned.copy_(x)
    wide = torch.empty(r, 2 * c, dtype=x.dtype, device="cuda")
    strided = wide[:, ::2]
    strided.copy_(x)
    transposed = x.t().contiguous().t()
    assert misaligned.is_contiguous() and misaligned.data_ptr() % 16 and not strided.is_contiguous() and not transposed.is_contiguous()
    want = S.quantize_bits(b, dtype, "mxfp6_e3m2", "ceil", 77, 78, axis)
    counter = "mx_sr_launch" if axis == -1 else "mx_sr_cols_launch"
    for t in (misaligned, strided, transposed):
        before = dict(ops.mx_counts)
        y = ops.mx_quantize_sr(t, "mxfp6_e3m2", 77, 78, "ceil", axis)
        assert y.shape == t.shape and y.is_contiguous()
        assert delta(before) == {"mx_copy_route": 1, counter: 1}
        assert_bits_equal(to_bits(y, dtype), want, dtype)


def test_the_refused_column_shape_raises_on_the_device_too():
    x = torch.zeros(64, 12, dtype=torch.bfloat16, device="cuda")
    before = dict(ops.mx_counts)
    with pytest.raises(ValueError, match="whole 16-byte vectors"):
        ops.mx_quantize_sr(x, "mxfp4", 1, axis=-2)
    assert ops.mx_counts == before
    assert ops.mx_quantize_sr(torch.zeros(0, 64, device="cuda"), "mxfp4", 1).shape == (0, 64) and ops.mx_counts == before      # empty: no launch


# ---- the public function ------------------------------------------------------------------------------------------------------------------------------

def test_gradient_of_the_public_function_is_the_incoming_tensor():
    x = from_bits(rand_bits((64, 96), "bf16", 31), "bf16").requires_grad_(True)
    for axis in (-1, -2):
        y = llm_qat_amd.mx_quantize_sr(x, "mxfp4", 5, 9, "ceil", axis)
        assert_same_bits(y.detach(), ops.mx_quantize_sr(x.detach(), "mxfp4", 5, 9, "ceil", axis))
        g = torch.randn_like(y)
        before = dict(ops.mx_counts)
        (gx,) = torch.autograd.grad(y, x, g)
        assert ops.mx_counts == before                  # no launch backward
        assert_same_bits(gx, g)


def test_two_replays_of_a_captured_launch_repeat_their_noise():
    """seed and stream are arguments of the captured launch: a replay draws the same numbers (the stated limit of graph capture)"""
    x = from_bits(rand_bits((64, 256), "bf16", 41), "bf16")
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mx_quantize_sr(static, "mxfp4", 3, 4)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mx_quantize_sr(static, "mxfp4", 3, 4)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_same_bits(first, out)
    assert_same_bits(first, ops.mx_quantize_sr(x, "mxfp4", 3, 4))
    assert not torch.equal(first, ops.mx_quantize_sr(x, "mxfp4", 3, 5))


# ---- QuantizeLinear(mx_backward_rounding=...) ---------------------------------------------------------------------------------------------------------

IN, OUT = 128, 96
WF, AF = "mxfp4", "mxfp8_e4m3"
SEED = 0xC0FFEE0123456789


class ReferenceLinear(torch.autograd.Function):
    """DESIGN.md sections 17 and 19 restated on the ops API: the same torch.matmul calls on operands of the same values, shapes and
    strides; streams: the stream ids of Qr(g) and Qc(g), or None for nearest rounding"""

    @staticmethod
    def forward(ctx, x, w, rule, fb, streams):
        ctx.save_for_backward(x, w)
        ctx.cfg = (rule, fb, streams)
        return F.linear(ops.mx_quantize(x, AF, scale_rule=rule), ops.mx_quantize(w, WF, scale_rule=rule))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        rule, fb, streams = ctx.cfg

        def qg(t, axis, k):
            if streams is None:
                return ops.mx_quantize_axis(t, fb, scale_rule=rule, axis=axis)
            return ops.mx_quantize_sr(t, fb, SEED, streams[k], rule, axis)
        with torch.autocast("cuda", enabled=False):
            d = g.dtype
            g2 = g.reshape(-1, OUT).contiguous()
            x2 = x.reshape(-1, IN).to(d)
            gx2 = torch.matmul(qg(g2, -1, 0), ops.mx_quantize_axis(w.to(d), fb, scale_rule=rule, axis=-2))
            pad = -g2.shape[0] % 32
            if pad:
                g2 = torch.cat([g2, g2.new_zeros(pad, OUT)])
                x2 = torch.cat([x2, x2.new_zeros(pad, IN)])
            gw = torch.matmul(qg(g2, -2, 1).t(), ops.mx_quantize_axis(x2, fb, scale_rule=rule, axis=-2))
        return gx2.reshape(x.shape).to(x.dtype), gw.to(w.dtype), None, None, None


MODES = {"bf16": (torch.bfloat16, False), "fp32": (torch.float32, False), "autocast": (torch.float32, True)}


def make_layer(pdt, rule, fb, rounding, g):
    layer = QuantizeLinear(IN, OUT, w_bits=4, a_bits=8, weight_format=WF, act_format=AF, mx_scale_rule=rule, mx_backward_format=fb,
                           mx_backward_rounding=rounding).cuda().to(pdt)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(OUT, IN, device="cuda", generator=g) * 0.1)
    return layer


@pytest.fixture
def sr_state():
    """the process seed and stream counter, put back afterwards"""
    from llm_qat_amd import utils_quant
    saved = dict(utils_quant._sr_state)
    yield utils_quant._sr_state
    utils_quant._sr_state.update(saved)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("fb", ["mxfp4", "mxfp8_e4m3"])
@pytest.mark.parametrize("mode", list(MODES))
def test_module_backward_matches_the_reference(mode, fb, rule, sr_state):
    pdt, autocast = MODES[mode]
    g = torch.Generator(device="cuda").manual_seed(5)
    layer = make_layer(pdt, rule, fb, "stochastic", g)
    llm_qat_amd.mx_sr_seed(SEED)
    stream = 0
    for shape in ((64, IN), (40, IN), (2, 20, IN)):
        x = torch.randn(shape, device="cuda", generator=g).to(pdt).requires_grad_(True)
        xr = x.detach().clone().requires_grad_(True)
        wr = layer.weight.detach().clone().requires_grad_(True)
        layer.weight.grad = None
        with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
            before = dict(ops.mx_counts)
            out = layer(x)
            assert delta(before) == {"mx_launch": 2}                     # the forward is unchanged in launches ...
            ref_out = ReferenceLinear.apply(xr, wr, rule, fb, (stream, stream + 1))
        assert out.dtype is (torch.bfloat16 if autocast else pdt)
        assert_same_bits(out.detach(), ref_out.detach())                 # ... and in values
        r = torch.randn(out.shape, device="cuda", generator=g).to(out.dtype)
        tokens = out.numel() // OUT
        before = dict(ops.mx_counts)
        out.backward(r)
        want = {"mx_sr_launch": 1, "mx_sr_cols_launch": 1, "mx_cols_launch": 2}      # one row-kernel and three column-kernel launches, as nearest
        if tokens % 32:
            want["mx_copy_route"] = 1                                    # the zero rows that pad the tokens
        assert delta(before) == want
        assert sr_state["next"] == stream + 2                            # Qr(g), then Qc(g)
        ref_out.backward(r)
        stream += 2
        assert x.grad.dtype is pdt and layer.weight.grad.dtype is pdt
        assert_same_bits(x.grad, xr.grad)
        assert_same_bits(layer.weight.grad, wr.grad)
        assert bool(x.grad.isfinite().all()) and bool(layer.weight.grad.isfinite().all()) and float(layer.weight.grad.abs().max()) > 0


def test_a_frozen_operand_draws_no_stream(sr_state):
    g = torch.Generator(device="cuda").manual_seed(6)
    layer = make_layer(torch.bfloat16, "floor", "mxfp8_e4m3", "stochastic", g)
    x = torch.randn(64, IN, device="cuda", dtype=torch.bfloat16)
    llm_qat_amd.mx_sr_seed(SEED)
    layer.weight.requires_grad_(False)                  # a frozen weight: no Qc(g), no Qc(x)
    out = layer(x.clone().requires_grad_(True))
    before = dict(ops.mx_counts)
    out.backward(torch.ones_like(out))
    assert delta(before) == {"mx_sr_launch": 1, "mx_cols_launch": 1} and sr_state["next"] == 1
    layer.weight.requires_grad_(True)                   # an input that needs none: no Qr(g), no Qc(W)
    out = layer(x)
    before = dict(ops.mx_counts)
    out.backward(torch.ones_like(out))
    assert delta(before) == {"mx_sr_cols_launch": 1, "mx_cols_launch": 1} and sr_state["next"] == 2
    want = torch.matmul(ops.mx_quantize_sr(torch.ones(64, OUT, device="cuda", dtype=torch.bfloat16), "mxfp8_e4m3", SEED, 1, axis=-2).t(),
                        ops.mx_quantize_axis(x, "mxfp8_e4m3", axis=-2))
    assert_same_bits(layer.weight.grad, want)


def test_a_seed_reproduces_and_the_counter_moves_on(sr_state):
    g = torch.Generator(device="cuda").manual_seed(7)
    layer = make_layer(torch.bfloat16, "ceil", "mxfp4", "stochastic", g)
    x = torch.randn(64, IN, device="cuda", generator=g).to(torch.bfloat16)
    r = torch.randn(64, OUT, device="cuda", generator=g).to(torch.bfloat16)

    def grads():
        xi = x.clone().requires_grad_(True)
        layer.weight.grad = None
        layer(xi).backward(r)
        return xi.grad.clone(), layer.weight.grad.clone()

    llm_qat_amd.mx_sr_seed(123)
    a = grads()
    b = grads()                                          # no reset: the next two stream ids
    assert llm_qat_amd.mx_sr_seed(123) == 123
    c = grads()
    assert_same_bits(a[0], c[0])
    assert_same_bits(a[1], c[1])
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    llm_qat_amd.mx_sr_seed(124)
    d = grads()
    assert not torch.equal(a[0], d[0]) and not torch.equal(a[1], d[1])
    sr_state.update(seed=None, next=0)                   # never seeded: the first stochastic backward takes torch's seed
    grads()
    assert sr_state["seed"] == torch.initial_seed() & U64 and sr_state["next"] == 2


@pytest.mark.parametrize("rounding", [None, "nearest"])
def test_nearest_and_none_are_the_existing_path(rounding, sr_state):
    assert (parent.IN, parent.OUT, parent.WF, parent.AF) == (IN, OUT, WF, AF)
    g = torch.Generator(device="cuda").manual_seed(8)
    layer = make_layer(torch.bfloat16, "floor", "mxfp4", rounding, g)
    x = torch.randn(40, IN, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    wr = layer.weight.detach().clone().requires_grad_(True)
    llm_qat_amd.mx_sr_seed(SEED)
    out = layer(x)
    ref_out = parent.ReferenceLinear.apply(xr, wr, "floor", "mxfp4")       # the row-axis API and transposes alone
    assert_same_bits(out.detach(), ref_out.detach())
    r = torch.randn(out.shape, device="cuda", generator=g).to(out.dtype)
    before = dict(ops.mx_counts)
    out.backward(r)
    assert delta(before) == {"mx_launch": 1, "mx_cols_launch": 3, "mx_copy_route": 1} and sr_state["next"] == 0
    ref_out.backward(r)
    assert_same_bits(x.grad, xr.grad)
    assert_same_bits(layer.weight.grad, wr.grad)
