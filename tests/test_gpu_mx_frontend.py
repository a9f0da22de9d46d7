"""The MX front-end's one quantizer path on the MI355X (ops._mx_quantize, utils_quant._MXQuantizer / _mx_apply, compiled.mx_fake_quant /
mx_export): every served combination of axis, rotation, scale rule and gradient, eager and compiled, gives the bits of the C entry point
called straight through _lib.lib() on the same input, with exactly the launches it is documented to make (ops.mx_counts).

The shapes are the smallest at which a route can go wrong: three dimensions, one and two rotation runs, a partial column tile, and a
bf16 row of 136 bytes, which the column kernel does not take (the transposed fallback)."""
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.mx_inference import MXLinear

pytestmark = pytest.mark.gpu

FMT = "mxfp4"
BF16, F32 = torch.bfloat16, torch.float32
ROW, COLS, FALLBACK = {"mx_launch": 1}, {"mx_cols_launch": 1}, {"mx_copy_route": 1, "mx_launch": 1}
CASES = [   # axis, shape, dtype, the forward's launches
    (-1, (3, 2, 128), BF16, ROW),
    (-1, (2, 64), F32, ROW),
    (-2, (2, 64, 72), BF16, COLS),       # nine 16-byte strips: a partial tile
    (-2, (32, 68), F32, COLS),
    (-2, (32, 68), BF16, FALLBACK),      # 136-byte rows are not whole 16-byte vectors
]
CELLS = [(rotate, rule, ste) for rotate in (False, True) for rule in ("floor", "ceil") for ste in ("identity", "clip")]


def served(axis, cell):
    return axis == -1 or (not cell[0] and cell[2] == "identity")


def delta(before):
    return {k: v - before[k] for k, v in ops.mx_counts.items() if v != before[k]}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous() and torch.equal(a.view(torch.uint8), b.contiguous().view(torch.uint8))


def make_input(axis, shape, dtype, seed=0):
    """random values over a few binades; the first block along `axis` is ones under a leading 1.96875 * 8, which "floor" saturates"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=gen) * torch.exp2(torch.randint(-3, 4, shape, generator=gen).float())
    xt = x if axis == -1 else x.transpose(-1, -2)
    first = xt.reshape(-1, xt.shape[-1])[0] if axis == -1 else xt[..., 0, :]     # (views: the writes land in x)
    first[..., :32] = 1.0
    first[..., 0] = 1.96875 * 8
    return x.to(dtype).cuda()


def flags_of(rotate, rule):
    return (_lib.MX_FLAG_ROTATE if rotate else 0) | (_lib.MX_FLAG_CEIL if rule == "ceil" else 0)


def rows_cols(t):
    return t.numel() // t.shape[-1], t.shape[-1]


def direct_rows(x, rotate, rule, want_mask):
    """fq_mx_fwd_ex on a contiguous x -> (y, mask | None)"""
    y = torch.empty_like(x)
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) if want_mask else None
    rc = _lib.lib().fq_mx_fwd_ex(x.data_ptr(), y.data_ptr(), mask.data_ptr() if want_mask else None, *rows_cols(x), ops.MX_FORMATS[FMT],
                                 ops._DTYPES[x.dtype], flags_of(rotate, rule), ops._stream(x))
    assert rc == 0
    return y, mask


def direct_forward(x, axis, route, rotate, rule, want_mask):
    """the entry point the route is documented to reach, on the same input"""
    assert x.is_contiguous() and x.data_ptr() % 16 == 0
    if axis == -1:
        return direct_rows(x, rotate, rule, want_mask)
    if route == FALLBACK:
        return direct_rows(x.transpose(-1, -2).contiguous(), False, rule, False)[0].transpose(-1, -2).contiguous(), None
    y = torch.empty_like(x)
    rc = _lib.lib().fqt_mx_fwd_cols(x.data_ptr(), y.data_ptr(), *rows_cols(x), ops.MX_FORMATS[FMT], ops._DTYPES[x.dtype], flags_of(False, rule),
                                    ops._stream(x))
    assert rc == 0
    return y, None


def direct_backward(g, mask, rotate):
    """identity: g itself, or fq_block_rotate of it; under a bitmap: fq_mx_ste_bwd"""
    L, dt, st = _lib.lib(), ops._DTYPES[g.dtype], ops._stream(g)
    if mask is None and not rotate:
        return g
    gx = torch.empty_like(g)
    if mask is None:
        assert L.fq_block_rotate(g.data_ptr(), gx.data_ptr(), *rows_cols(g), dt, st) == 0
    else:
        assert L.fq_mx_ste_bwd(g.data_ptr(), mask.data_ptr(), gx.data_ptr(), *rows_cols(g), dt, _lib.MX_FLAG_ROTATE if rotate else 0, st) == 0
    return gx


def quantizer(axis, cell):
    rotate, rule, ste = cell
    return lambda t: llm_qat_amd.mx_quantize_axis(t, FMT, rotate=rotate, scale_rule=rule, ste=ste, axis=axis)


def step(fn, x, g):
    """forward + backward of fn on a leaf over x -> (y, grad, the forward's launches, the backward's, the node's name and what it saved)"""
    leaf = x.detach().requires_grad_(True)
    before = dict(ops.mx_counts)
    y = fn(leaf)
    fwd = delta(before)
    node = (type(y.grad_fn).__name__, len(getattr(y.grad_fn, "saved_tensors", ())))       # (read before the backward frees them)
    before = dict(ops.mx_counts)
    (gx,) = torch.autograd.grad(y, leaf, g)
    return y, gx, fwd, delta(before), node


@pytest.mark.parametrize("mode", ["eager", "compiled"])
@pytest.mark.parametrize("axis, shape, dtype, route", CASES, ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, dict) else "+".join(v))
def test_every_served_cell_gives_the_entry_points_bits_and_launches(axis, shape, dtype, route, mode):
    x = make_input(axis, shape, dtype)
    g = torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(1)).to(dtype).cuda()
    clipped = False
    for cell in CELLS:
        if not served(axis, cell):
            with pytest.raises(ValueError, match="column axis"):
                quantizer(axis, cell)(x)
            continue
        rotate, rule, ste = cell
        clip = ste == "clip"
        want_y, mask = direct_forward(x, axis, route, rotate, rule, clip)
        want_gx = direct_backward(g, mask, rotate)
        fn = quantizer(axis, cell)
        if mode == "compiled":
            torch._dynamo.reset()
            fn = torch.compile(fn, backend="aot_eager", fullgraph=True)
        y, gx, fwd, bwd, node = step(fn, x, g)
        assert same_bits(y.detach(), want_y), (cell, "forward")
        assert same_bits(gx, want_gx), (cell, "gradient")
        assert fwd == dict(route, **({"mx_mask_launch": 1} if clip else {})), (cell, fwd)
        assert bwd == ({"mx_ste_launch": 1} if clip else {"mx_rotate_launch": 1} if rotate else {}), (cell, bwd)
        if mode == "eager":
            assert node == ("_MXQuantizerBackward", 1 if clip else 0), node
        if clip and not rotate and rule == "floor":
            clipped = bool(((want_gx == 0) & (g != 0)).any())
            assert clipped                                         # the bitmap does clip the saturated leading value
        if mode == "eager":                                        # without a gradient to come no bitmap is written
            before = dict(ops.mx_counts)
            assert same_bits(fn(x), want_y) and delta(before) == route
    assert clipped or axis == -2


@pytest.mark.parametrize("axis, shape, dtype", [(-1, (4, 128), BF16), (-2, (64, 72), BF16)])
def test_a_strided_or_misaligned_input_takes_exactly_one_copy(axis, shape, dtype):
    x = make_input(axis, shape, dtype)
    want = direct_forward(x, axis, ROW if axis == -1 else COLS, False, "floor", False)[0]
    wide = torch.zeros(shape[0], shape[1] * 2, dtype=dtype, device="cuda")
    strided = wide[:, ::2]
    strided.copy_(x)
    flat = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
    shifted = flat[1:1 + x.numel()].view(shape)                   # contiguous, 2 bytes off a 16-byte boundary
    shifted.copy_(x)
    assert not strided.is_contiguous() and shifted.is_contiguous() and shifted.data_ptr() % 16 == 2
    for t in (strided, shifted):
        for f in (ops.mx_quantize_axis, llm_qat_amd.mx_quantize_axis):
            before = dict(ops.mx_counts)
            y = f(t, FMT, axis=axis)
            assert delta(before) == {"mx_copy_route": 1, "mx_launch": 1}      # (along axis -2 the copy is the transposed one)
            assert same_bits(y, want)
    if axis == -1:          # the bitmap of mx_ste_backward takes the same one copy
        y, mask = ops.mx_quantize(x, FMT, return_mask=True)
        g = torch.ones_like(x)
        want_gx = direct_backward(g, mask, False)
        buf = torch.zeros(mask.numel() + 16, dtype=torch.uint8, device="cuda")
        off = buf[1:1 + mask.numel()]
        off.copy_(mask)
        before = dict(ops.mx_counts)
        assert same_bits(ops.mx_ste_backward(g, off), want_gx)
        assert delta(before) == {"mx_copy_route": 1, "mx_ste_launch": 1}


@pytest.mark.parametrize("axis, shape", [(-1, (0, 64)), (-1, (3, 0)), (-2, (0, 32, 8)), (-2, (32, 0)), (-2, (0, 8))])
def test_an_empty_tensor_moves_no_counter(axis, shape):
    x = torch.empty(shape, dtype=BF16, device="cuda", requires_grad=True)
    before = dict(ops.mx_counts)
    y = llm_qat_amd.mx_quantize_axis(x, FMT, axis=axis)
    y.sum().backward()
    z = ops.mx_quantize_axis(x.detach(), FMT, scale_rule="ceil", axis=axis)
    assert delta(before) == {}
    assert y.shape == z.shape == x.shape and y.dtype == z.dtype == BF16 and x.grad.shape == x.shape
    if axis == -1:
        e = ops.mx_export(x.detach(), FMT)
        r = ops.mx_rotate(torch.empty(0, 64, dtype=BF16, device="cuda"))
        assert delta(before) == {} and e.scales.shape == shape[:-1] + (shape[-1] // 32,) and r.shape == (0, 64)


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("rule", ["floor", "ceil"])
def test_mx_linear_compiled_is_one_export_and_one_gemm_launch(rotate, rule):
    torch.manual_seed(5)
    m = MXLinear(128, 32, rotate=rotate, scale_rule=rule, bias=True, dtype=BF16).cuda()
    w = ops.mx_export(torch.randn(32, 128, device="cuda").bfloat16(), "mxfp4", rotate=rotate, scale_rule=rule)
    m.weight_elements.copy_(w.elements)
    m.weight_scales.copy_(w.scales)
    m.bias.copy_(torch.randn(32))
    x = make_input(-1, (3, 128), BF16, seed=2)
    with torch.no_grad():
        before = dict(ops.mx_counts)
        want = m(x)
        assert delta(before) == {"mx_export_launch": 1, "mx_gemm_launch": 1, "mx_gemm_skinny": 1}
        torch._dynamo.reset()
        cm = torch.compile(m, backend="aot_eager", fullgraph=True)
        before = dict(ops.mx_counts)
        got = cm(x)
        assert delta(before) == {"mx_export_launch": 1, "mx_gemm_launch": 1, "mx_gemm_skinny": 1}
    assert same_bits(got, want)
    a = ops.mx_export(x, "mxfp8_e4m3", rotate=rotate, scale_rule=rule)
    by_hand = ops.mx_matmul(a, m.weight_export(), out_dtype=BF16) + m.bias
    assert same_bits(want, by_hand)


def test_a_misaligned_gemm_operand_is_copied_once_and_not_counted():
    w = ops.mx_export(make_input(-1, (32, 128), BF16, seed=3), "mxfp4")
    a = ops.mx_export(make_input(-1, (2, 128), BF16, seed=4), "mxfp8_e4m3")
    want = ops.mx_matmul(a, w)
    buf = torch.zeros(a.elements.numel() + 16, dtype=torch.uint8, device="cuda")
    off = buf[1:1 + a.elements.numel()].view(a.elements.shape)
    off.copy_(a.elements)
    assert off.data_ptr() % 16 == 1
    before = dict(ops.mx_counts)
    got = ops.mx_matmul_tensors(off, a.scales, a.fmt, w.elements, w.scales, w.fmt, a.shape, BF16)
    assert delta(before) == {"mx_gemm_launch": 1, "mx_gemm_skinny": 1}
    assert same_bits(got, want)
