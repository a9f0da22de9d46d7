"""The front-end's one launch helper (ops._launch: the tensor's device current, its current stream last) and what was folded onto it: the
side stream, a second device, the MX entry points (ops.mx_quantize / mx_export now always call the *_ex symbols) and the one merged
_MXQuantizer Function.  Every comparison is bit for bit."""
import pytest
import torch

from llm_qat_amd import _lib, ops
from llm_qat_amd import utils_quant as UQ

pytestmark = pytest.mark.gpu

LO, HI = -2.0, 2.0


def make_inputs(device):
    """x [5, 256], w [3, 256], two gradients, bf16 -- x comes out of a kernel launched on the CURRENT stream just before it is used, into
    memory the stream's allocator hands out fresh: a launch that went to another stream would read it too early"""
    gen = torch.Generator(device="cpu").manual_seed(5)
    a = torch.randn(512, 512, generator=gen).to(device)
    rest = [t.to(device) for t in (torch.randn(3, 256, generator=gen).bfloat16(), torch.randn(5, 256, generator=gen).bfloat16(),
                                   torch.randn(3, 256, generator=gen).bfloat16())]
    x = ((a @ a)[:5, :256] * 0.05).bfloat16()
    return (x, *rest)


def run_calls(x, w, gx, gw, after=lambda: None):
    """each front-end path once, `after()` behind every call -> the tensors that must not depend on the stream or on which device is
    current (a side buffer's bounds are compared; its bitmap only through the gradients it masks: rows that cannot clip leave theirs
    unwritten)"""
    def call(fn, *args, **kw):
        res = fn(*args, **kw)
        after()
        return res
    out = [call(ops.sym_quantize, x, 8)]
    y, side, rows, cols = call(ops.train_forward, "sym", x, 8, False, LO, HI)
    out += [y, ops.split_side(side, rows)[0], call(ops.train_backward, gx, side, rows, cols, LO, HI)]
    wq, xq, side_w, side_x, rows_w, rows_x, cols = call(ops.pair_forward, w, x, 4, 8, LO, HI, True, True)
    out += [wq, xq, ops.split_side(side_w, rows_w)[0], ops.split_side(side_x, rows_x)[0]]
    out += list(call(ops.pair_backward, gw, gx, side_w, side_x, rows_w, rows_x, cols, LO, HI))
    y, side, rows, cols = call(ops.group_forward, "sym", x, 8, 64, lo=LO, hi=HI, train=True)
    out += [y, ops.split_side(side, rows)[0], call(ops.train_backward, gx, side, rows, cols, LO, HI)]
    out.append(call(ops.mx_quantize, x, "mxfp4"))
    return out


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu()), f"result {i} differs"


@pytest.fixture(scope="module")
def on_default_stream():
    got = run_calls(*make_inputs("cuda:0"))
    torch.cuda.synchronize()
    return got


def test_side_stream(on_default_stream):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run_calls(*make_inputs("cuda:0"))
    s.synchronize()
    assert_same(got, on_default_stream)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_second_device_while_the_first_is_current():
    def still_on_0():
        assert torch.cuda.current_device() == 0

    with torch.cuda.device(1):
        want = run_calls(*make_inputs("cuda:1"))
        torch.cuda.synchronize()
    still_on_0()
    x, w, gx, gw = make_inputs("cuda:1")
    got = run_calls(x, w, gx, gw, after=still_on_0)
    torch.cuda.synchronize(1)
    assert all(t.device == x.device for t in got)
    assert_same(got, want)
    for refused in (lambda: ops.sym_quantize(x, 0), lambda: ops.train_forward("sym", x, 0, False, LO, HI)):
        with pytest.raises(ValueError):
            refused()
        assert torch.cuda.current_device() == 0


def mx_input(dtype):
    """[3, 128]: block 0 holds a NaN, block 1 is all zeros, block 2's leading value (1.96875 * 2^3 among ones) saturates under "floor" for
    every format; the rest is random"""
    gen = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(3, 128, generator=gen)
    x[0, 5] = float("nan")
    x[0, 32:64] = 0.0
    x[0, 64:96] = 1.0
    x[0, 64], x[0, 71] = 1.96875 * 8, -1.96875 * 8
    return x.to(dtype).cuda()


def counts_delta(before):
    return {k: v - before[k] for k, v in ops.mx_counts.items() if v != before[k]}


@pytest.mark.parametrize("fmt", list(ops.MX_FORMATS))
def test_mx_entry_points_are_the_older_symbols_byte_for_byte(fmt):
    L = _lib.lib()
    code = ops.MX_FORMATS[fmt]
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        x = mx_input(dtype)
        rows, cols = x.shape
        dt, st = ops._DTYPES[dtype], ops._stream(x)
        for rotate in (False, True):
            want = torch.empty_like(x)
            assert (L.fq_mx_fwd_rot if rotate else L.fq_mx_fwd)(x.data_ptr(), want.data_ptr(), rows, cols, code, dt, st) == 0
            before = dict(ops.mx_counts)
            got = ops.mx_quantize(x, fmt, rotate)
            assert counts_delta(before) == {"mx_launch": 1}
            assert got.dtype == dtype and got.shape == x.shape
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), (fmt, dtype, rotate)
            if fmt.startswith("mxfp6"):
                continue
            elems = torch.empty(rows, cols // 2 if fmt == "mxfp4" else cols, dtype=torch.uint8, device="cuda")
            scales = torch.empty(rows, cols // 32, dtype=torch.uint8, device="cuda")
            assert (L.fq_mx_export_rot if rotate else L.fq_mx_export)(x.data_ptr(), elems.data_ptr(), scales.data_ptr(), rows, cols, code, dt, st) == 0
            before = dict(ops.mx_counts)
            e = ops.mx_export(x, fmt, rotate)
            assert counts_delta(before) == {"mx_export_launch": 1}
            assert torch.equal(e.elements, elems) and torch.equal(e.scales, scales), (fmt, dtype, rotate)
            assert e.rotated is rotate


def saturating(dtype=torch.bfloat16):
    x = torch.ones(2, 64, dtype=dtype, device="cuda")
    x[:, 0], x[1, 40] = 1.96875 * 8, -1.96875 * 8
    return x


def test_merged_mx_quantizer_defaults_save_nothing_and_pass_the_gradient_through():
    x = saturating().requires_grad_(True)
    g = torch.randn(2, 64, device="cuda").bfloat16()
    y = UQ.mx_quantize(x, "mxfp4")
    assert type(y.grad_fn).__name__ == "_MXQuantizerBackward" and y.grad_fn.saved_tensors == ()
    assert torch.equal(y, ops.mx_quantize(x.detach(), "mxfp4"))
    y.backward(g)
    assert torch.equal(x.grad.view(torch.int16), g.view(torch.int16))


def test_merged_mx_quantizer_rotated_gradient_is_the_rotated_gradient():
    x = saturating().requires_grad_(True)
    g = torch.randn(2, 64, device="cuda").bfloat16()
    y = UQ.mx_quantize(x, "mxfp4", rotate=True)
    assert type(y.grad_fn).__name__ == "_MXQuantizerBackward" and y.grad_fn.saved_tensors == ()
    y.backward(g)
    assert torch.equal(x.grad.view(torch.int16), ops.mx_rotate(g).view(torch.int16))


@pytest.mark.parametrize("rotate", [False, True])
def test_merged_mx_quantizer_clip_gradient_is_the_masked_one(rotate):
    x = saturating().requires_grad_(True)
    g = torch.randn(2, 64, device="cuda").bfloat16()
    want_y, mask = ops.mx_quantize(x.detach(), "mxfp4", rotate=rotate, return_mask=True)
    y = UQ.mx_quantize(x, "mxfp4", rotate=rotate, ste="clip")
    assert type(y.grad_fn).__name__ == "_MXQuantizerBackward" and torch.equal(y, want_y)
    assert len(y.grad_fn.saved_tensors) == 1 and torch.equal(y.grad_fn.saved_tensors[0], mask)
    y.backward(g)
    want = ops.mx_ste_backward(g, mask, rotate)
    assert torch.equal(x.grad.view(torch.int16), want.view(torch.int16))
    assert rotate or (want == 0).any()        # the mask does clip something (unrotated: the saturated leading values)
