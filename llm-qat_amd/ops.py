"""Functional front-end over the C ABI: torch tensors in, torch tensors out.

Everything here is host-side plumbing (shape -> [rows, cols], dtype codes, stream handle,
workspace); the arithmetic happens in the HIP kernels.  CPU tensors are rejected: this
package is the MI355X path and has no CPU implementation.
"""
import ctypes
import os

import torch

from . import _lib

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16, torch.float64: _lib.DTYPE_F64}
_SEM_NAMES = {"cpu_eager": _lib.SEM_CPU_EAGER, "device_eager": _lib.SEM_DEVICE_EAGER}
# Default since round 5: a CUDA tensor gets what the reference computes ON A GPU ("device_eager": ATen's GPU kernels keep an added Python
# scalar in fp32 and turn `.div(python scalar)` into a multiply by the fp32 reciprocal) -- the drop-in runs on the GPU, so that is the
# arithmetic it replaces; pinned to the reference's own code by tests/golden/device_scalars.npz and to live ATen on the MI355X
# (tests/test_gpu_device_scalars.py).  "cpu_eager" (the reference run on CPU tensors, the arithmetic of the round-1 fixtures) stays a switch;
# CPU tensors served through allow_cpu_tensors() run ATen's own CPU kernels and are not affected by either.
_semantics = _SEM_NAMES[os.environ.get("LLMQAT_AMD_SEMANTICS", "device_eager")]


def set_semantics(name):
    """'device_eager' (default: bit-equal to the reference's eager ops run on a GPU, outside autocast) or 'cpu_eager' (bit-equal to the
    reference run on CPU).  They differ only for bf16 rows whose |max| is below ~3e-4, fp16 rows with |max| in [2^-13, 2^-12) and for
    fp32 AsymQuantizer (DESIGN.md "Numerics"); under autocast the arithmetic is the device's either way."""
    global _semantics
    _semantics = _SEM_NAMES[name]


def get_semantics():
    return "device_eager" if _semantics == _lib.SEM_DEVICE_EAGER else "cpu_eager"


# Under torch.autocast("cuda") the reference runs on the device by definition, where ATen keeps the `+ 1e-6` scalar in fp32: the
# autocast arithmetic is always launched with device-eager scalars (the C ABI takes `sem` there too: the parity tests drive both).
_SEM_AUTOCAST = _lib.SEM_DEVICE_EAGER


def rows_cols(shape, layerwise):
    """Granularity rules of utils_quant.py:50-70 -> the [rows, cols] view the kernels take."""
    n = 1
    for d in shape:
        n *= d
    if layerwise:
        return 1, n
    nd = len(shape)
    if nd <= 3:
        cols = shape[-1] if nd else 1
        return (n // cols if cols else 0), cols
    if nd == 4:
        return shape[0] * shape[1], shape[2] * shape[3]
    raise ValueError(f"fake-quant expects at most 4 dimensions, got {nd}")  # utils_quant.py:70


def bits_arg(num_bits):
    """`num_bits` as the Python int the kernels take.  The reference computes `2 ** (num_bits - 1) - 1` in Python and then
    `int / Tensor` (= reciprocal * int, models/utils_quant.py:71), so an integral float means the same thing; a NON-integral float would
    mean a fractional number of levels and a TENSOR would turn that line into a true Tensor / Tensor division (different roundings) --
    neither is what any caller of the reference passes, and neither is served: refused loudly rather than silently truncated."""
    if isinstance(num_bits, torch.Tensor):
        raise TypeError("num_bits must be a Python int (a tensor changes the reference's arithmetic to a true division: not served)")
    b = int(num_bits)
    if b != num_bits:
        raise ValueError(f"num_bits must be integral, got {num_bits!r}")
    return b


def _prep(x, what):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x).__name__}")
    if x.device.type != "cuda":
        raise RuntimeError(f"{what}: tensor is on '{x.device}'. llm_qat_amd runs on MI355X only and has no CPU "
                           "fallback; move the tensor to the GPU (or use the reference implementation on CPU).")
    code = _DTYPES.get(x.dtype)
    if code is None:
        raise NotImplementedError(f"{what}: dtype {x.dtype} is not supported (float32, bfloat16, float16, float64 are)")
    return code


# The raw current-stream handle / current device index straight from the C bindings (what Inductor's generated code uses):
# 0.2 us per call instead of the 2-3 us `torch.cuda.current_stream().cuda_stream` spends building a Stream object.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device
if _raw_stream is None:
    def _raw_stream(idx):
        return torch.cuda.current_stream(idx).cuda_stream


def _stream(x):
    """the current stream of x's device, as the `hipStream_t` the C ABI takes"""
    idx = x.device.index
    return _raw_stream(_cur_dev() if idx is None else idx)


def _launch(t, fn, *args):
    """fn(*args, stream) -> its status code, on the current stream of t's device; that device is made current for the call only where it
    is not already (and restored).  Every launch function of the C ABI takes the stream last."""
    cur = _cur_dev()
    idx = t.device.index
    if idx is None or idx == cur:
        return fn(*args, _raw_stream(cur))
    torch.cuda.set_device(idx)
    try:
        return fn(*args, _raw_stream(idx))
    finally:
        torch.cuda.set_device(cur)


def _served(rc, what):
    """status code of a launch -> True (done) | False (FQ_ERR_UNSUPPORTED: the caller takes its other route); anything else raises"""
    if rc:
        if rc == _lib.ERR_UNSUPPORTED:
            return False
        _lib.check(rc, what)
    return True


def _size_query(name):
    """a byte-size query of the C ABI over (rows, cols, dtype code), memoised"""
    memo = {}

    def query(rows, cols, code):
        k = (rows, cols, code)
        v = memo.get(k)
        if v is None:
            v = memo[k] = getattr(_lib.lib(), name)(rows, cols, code)
        return v
    return query


_ws_bytes = _size_query("fq_rowwise_workspace_bytes")
_mask_bytes = _size_query("fq_ste_mask_bytes")


# ---- the side buffer of a training forward: one uint8 allocation, float[rows][2] row bounds followed by the STE row bitmap.  The C++ node
# (csrc/fq_autograd_node.cpp) allocates and splits the same layout on its own: a change here is a change there.
SIDE_ROW_BYTES = 8   # one row's bounds: 2 floats


def _side_alloc(rows, mask_bytes, device):
    """-> (side, bounds pointer, mask pointer)"""
    side = torch.empty(rows * SIDE_ROW_BYTES + mask_bytes, dtype=torch.uint8, device=device)
    sp = side.data_ptr()
    return side, sp, sp + rows * SIDE_ROW_BYTES


_NO_SIDE = (None, None, None)   # what _side_alloc's callers pass for a tensor that records nothing


def _side_ptrs(side, rows):
    """-> (bounds pointer, mask pointer) of a side buffer"""
    sp = side.data_ptr()
    return sp, sp + rows * SIDE_ROW_BYTES


def split_side(side, rows):
    """A side buffer -> (bounds float32 [rows, 2], mask uint8), views of its storage."""
    n = rows * SIDE_ROW_BYTES
    return side[:n].view(torch.float32).view(rows, 2), side[n:]


def _contig(x):
    return x if x.is_contiguous() else x.contiguous()


def _like_input(x, xc, y):
    """y, computed from xc = _contig(x), in the layout the reference's elementwise ops give x's result (empty_like's strides)"""
    if xc is x:
        return y
    out = torch.empty_like(x, dtype=y.dtype)
    out.copy_(y)
    return out


def _empty_input(what, x, layerwise):
    """A tensor without elements, as the reference treats it (models/utils_quant.py:50-68 / :110-122; asked of the live reference):
    a reduction over NOTHING raises what torch raises there -- RuntimeError for the layerwise (whole-tensor) max, and for the 4-D
    branch's `view(d0, d1, -1)` when d0 * d1 == 0 (the -1 is then ambiguous); IndexError for an empty reduction dimension (the last
    one; d2 * d3 == 0 in the 4-D branch) -- while zero ROWS of a non-empty last dimension simply give an empty result."""
    if layerwise:
        raise RuntimeError(f"{what}: max(): Expected reduction dim to be specified for input.numel() == 0 (layerwise reduction of an empty tensor)")
    if x.dim() == 4:
        if x.shape[0] * x.shape[1] == 0:
            raise RuntimeError(f"{what}: cannot reshape tensor of 0 elements into shape [{x.shape[0]}, {x.shape[1]}, -1] because the unspecified "
                               "dimension size -1 can be any value and is ambiguous")
        raise IndexError(f"{what}: max(): Expected reduction dim 2 to have non-zero size.")
    if x.shape[-1] == 0:
        raise IndexError(f"{what}: max(): Expected reduction dim {x.dim() - 1} to have non-zero size.")


# ---- rows that do not follow one another in memory ("last dim contiguous, rows strided": slices, chunk(), transpose(0, 1) of a 3-D tensor)
# are served IN the kernels (the C ABI's fq_rows_view, ABI 5): no .contiguous() in front of the launch, no copy_ behind it, and the result
# keeps the layout the reference's elementwise ops give it (torch.empty_like's rule: the input's strides when it is dense, else contiguous).
# Anything else that is not contiguous -- a strided LAST dimension, 4-D views, layerwise -- keeps the copy path.
def rows_view(t, layerwise=False):
    """-> None: contiguous (no view needed) | (n_inner, stride_outer, stride_inner) in elements | False: needs a copy"""
    if t.is_contiguous():
        return None
    nd = t.dim()
    if layerwise or nd < 2 or nd > 3 or t.shape[-1] < 2 or t.stride(-1) != 1:
        return False
    if nd == 2:
        return (t.shape[0], 0, t.stride(0))
    return (t.shape[1], t.stride(0), t.stride(1))


def check_4d(x, layerwise):
    """the reference flattens a 4-D input with `input.view(d0, d1, -1)` (models/utils_quant.py:63 / :127): a layout for which that view does
    not exist raises there -- and here, with torch's own exception, instead of being served through a copy"""
    if x.dim() == 4 and not layerwise and not x.is_contiguous():
        x.view(x.shape[0], x.shape[1], -1)


def _rv(v):
    return _lib.RowsView(*v) if v else _lib.RowsView(0, 0, 0)


def _strided_out(x, dtype=None):
    """the result tensor for a strided input and its view: empty_like keeps a dense input's strides and makes everything else contiguous,
    exactly what the reference's elementwise ops (TensorIterator) do"""
    y = torch.empty_like(x) if dtype is None else torch.empty_like(x, dtype=dtype)
    return y, rows_view(y)


_views_served = 0   # launches that took a view instead of a copy (tests read it)


def _view_served():
    global _views_served
    _views_served += 1


def _rowwise(kind, x, num_bits, layerwise, want_bounds, debug):
    what = f"{kind}_quantize"
    code = _prep(x, what)
    rows, cols = rows_cols(tuple(x.shape), layerwise)
    if x.numel() == 0:
        _empty_input(what, x, layerwise)
        return torch.empty_like(x), None, None, None
    check_4d(x, layerwise)
    L = _lib.lib()
    xv = rows_view(x, layerwise)
    if xv and not debug and code != _lib.DTYPE_F64:   # strided rows: served in the kernel
        y, yv = _strided_out(x)
        if yv is not False:
            bounds = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if want_bounds else None
            rc = _launch(x, L.fq_rowwise_fwd_v, 1 if kind == "asym" else 0, x.data_ptr(), _rv(xv), y.data_ptr(), _rv(yv), rows, cols, int(num_bits), code,
                         _semantics, 0.0, 0.0, bounds.data_ptr() if want_bounds else None, None, 0)
            if _served(rc, what):
                _view_served()
                return y, bounds, None, None
    xc = _contig(x)
    y = torch.empty_like(xc)
    ws_bytes = _ws_bytes(rows, cols, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    ws_ptr = ws.data_ptr() if ws is not None else None
    bounds = idx = scale = None
    if code == _lib.DTYPE_F64:
        want_bounds = False   # float64: a correctness path without training-mode side buffers (the backward re-reads x)
    if debug:
        idx = torch.empty(xc.shape, dtype=torch.int32, device=x.device)
        scale = torch.empty((rows,) if kind == "sym" else (rows, 2), dtype=torch.float32, device=x.device)
        rc = _launch(x, L.fq_sym_fwd_debug if kind == "sym" else L.fq_asym_fwd_debug, xc.data_ptr(), y.data_ptr(), idx.data_ptr(), scale.data_ptr(),
                     rows, cols, int(num_bits), code, _semantics, ws_ptr, ws_bytes)
    else:
        if want_bounds:
            bounds = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        rc = _launch(x, L.fq_sym_fwd if kind == "sym" else L.fq_asym_fwd, xc.data_ptr(), y.data_ptr(), rows, cols, int(num_bits), code, _semantics,
                     bounds.data_ptr() if bounds is not None else None, ws_ptr, ws_bytes)
    _lib.check(rc, what)
    if idx is not None and xc is not x:
        idx = idx.reshape(x.shape)
    return _like_input(x, xc, y), bounds, idx, scale


# ---- lean path used by the autograd Functions: one side allocation (row bounds + STE mask), memoised sizes ----
def _aligned(g):
    """contiguous and 16-byte aligned (a gradient can be an offset view into a larger buffer)"""
    g = _contig(g)
    return g.clone() if g.data_ptr() & 15 else g


def _mask_slot(g, side, rows, inplace=False, out_dtype=None):
    """One tensor of a masked STE backward launch -> (g, gx, (g, gx, rows, bounds, mask) as the C ABI takes them): the gradient contiguous
    and 16-byte aligned, and fp32 behind a wide forward (out_dtype given); the result in place, fresh, or fresh in out_dtype; the side
    buffer's two pointers.  What train_backward, train_backward_wide, pair_backward, pair_backward_wide and multi_backward do per tensor."""
    if out_dtype is not None and g.dtype != torch.float32:
        g = g.float()
    g = g.contiguous()
    gp = g.data_ptr()
    if gp & 15:   # (a contiguous gradient can still be an offset view into a larger buffer)
        g = g.clone()
        gp = g.data_ptr()
    if inplace:
        gx = g
    elif out_dtype is None:
        gx = torch.empty_like(g)
    else:
        gx = torch.empty(g.shape, dtype=out_dtype, device=g.device)
    bp = side.data_ptr()
    return g, gx, (gp, gx.data_ptr(), rows, bp, bp + rows * SIDE_ROW_BYTES)


def train_forward(kind, x, num_bits, layerwise, lo, hi):
    """-> (y, side, rows, cols) or None.  `side` is one uint8 buffer: float[rows][2] bounds followed by the mask."""
    if x.device.type != "cuda":
        _prep(x, f"{kind}_quantize")
    code = _DTYPES.get(x.dtype)
    if code is None:
        _prep(x, f"{kind}_quantize")
    if x.numel() == 0:
        return None
    xv = None
    if not x.is_contiguous():
        check_4d(x, layerwise)
        xv = rows_view(x, layerwise)
        if not xv:
            return None
    rows, cols = rows_cols(tuple(x.shape), layerwise)
    mbytes = _mask_bytes(rows, cols, code)
    if not mbytes:
        return None
    L = _lib.lib()
    if xv:   # strided rows: served in the kernel (the side buffer is indexed by row number and stays dense)
        y, yv = _strided_out(x)
        if yv is False:
            return None
        side, bp, mp = _side_alloc(rows, mbytes, x.device)
        rc = _launch(x, L.fq_rowwise_fwd_v, 1 if kind == "asym" else 0, x.data_ptr(), _rv(xv), y.data_ptr(), _rv(yv), rows, cols, int(num_bits), code,
                     _semantics, lo, hi, bp, mp, mbytes)
        if not _served(rc, f"{kind}_quantize_train"):
            return None
        _view_served()
        return y, side, rows, cols
    y = torch.empty_like(x)
    side, bp, mp = _side_alloc(rows, mbytes, x.device)
    rc = _launch(x, L.fq_sym_fwd_train if kind == "sym" else L.fq_asym_fwd_train, x.data_ptr(), y.data_ptr(), rows, cols, int(num_bits), code, _semantics,
                 lo, hi, bp, mp, mbytes)
    if rc and not _served(rc, f"{kind}_quantize_train"):   # (`rc and`: the served call builds no message)
        return None
    return y, side, rows, cols


def _mask_backward_v(gs, sides, rows, cols, lo, hi, code, wide, inplace=None, out_dtype=None):
    """fq_ste_bwd_mask_multi_v over 1..2 gradients of which at least one has strided rows -> [gx] or None (not served: copy path)"""
    n = len(gs)
    arr = (_lib.BwdTensorV * n)()
    outs = []
    for i, (g, sd, r) in enumerate(zip(gs, sides, rows)):
        gv = rows_view(g)
        if gv is False or g.data_ptr() & 15:
            return None
        if inplace and inplace[i]:
            o, ov = g, gv
        else:
            o, ov = _strided_out(g, out_dtype)
            if ov is False:
                return None
        outs.append(o)
        arr[i] = _lib.BwdTensorV(g.data_ptr(), o.data_ptr(), r, *_side_ptrs(sd, r), _rv(gv), _rv(ov))
    rc = _launch(gs[0], _lib.lib().fq_ste_bwd_mask_multi_v, n, arr, cols, float(lo), float(hi), code, 1 if wide else 0)
    if not _served(rc, "ste_backward_mask[strided]"):
        return None
    _view_served()
    return outs


def train_backward(grad_output, side, rows, cols, lo, hi, inplace=False):
    """inplace: mask the gradient where it stands and return it (fq_ste_bwd_mask with gx == g): rows that cannot clip are
    not touched, so a weight's gradient costs a launch and no traffic.  Only for callers that own grad_output exclusively."""
    code = _DTYPES.get(grad_output.dtype)
    if code is None or grad_output.device.type != "cuda":
        _prep(grad_output, "ste_backward")
    if not grad_output.is_contiguous() and grad_output.numel():   # strided rows: masked in the kernel, no .contiguous() copy
        res = _mask_backward_v([grad_output], [side], [rows], cols, lo, hi, code, False, [inplace])
        if res is not None:
            return res[0]
    g, gx, (gp, gxp, _, bp, mp) = _mask_slot(grad_output, side, rows, inplace)
    rc = _launch(g, _lib.lib().fq_ste_bwd_mask, gp, gxp, rows, cols, lo, hi, bp, mp, side.numel() - (mp - bp), code)   # (mp - bp: the bounds' bytes)
    if rc:
        _lib.check(rc, "ste_backward_mask")
    return gx


def train_backward_wide(grad_output, side, rows, cols, lo, hi, out_dtype):
    """STE backward behind a fp32-result (autocast) forward: fp32 grad_output -> masked gradient in the input's dtype
    (the autograd engine's cast folded in; fq_ste_bwd_mask_wide).  side = bounds + mask of THAT forward."""
    code = _DTYPES.get(out_dtype)
    if code is None or grad_output.device.type != "cuda":
        raise TypeError(f"ste_backward[wide]: unsupported input dtype {out_dtype} / device {grad_output.device}")
    if grad_output.dtype == torch.float32 and not grad_output.is_contiguous() and grad_output.numel():
        res = _mask_backward_v([grad_output], [side], [rows], cols, lo, hi, code, True, None, out_dtype)
        if res is not None:
            return res[0]
    g, gx, slot = _mask_slot(grad_output, side, rows, False, out_dtype)
    rc = _launch(g, _lib.lib().fq_ste_bwd_mask_wide, *slot, None, None, 0, None, None, cols, float(lo), float(hi), code)
    _lib.check(rc, "ste_backward_mask_wide")
    return gx


def autocast_active(x):
    """True when the reference's op chain would run its fp32-promoted arithmetic on x: a 16-bit CUDA tensor inside
    torch.autocast("cuda") (`reciprocal`, i.e. the `int / Tensor` of utils_quant.py:71, is on autocast's fp32 list)."""
    return x.dtype in (torch.bfloat16, torch.float16) and x.is_cuda and torch.is_autocast_enabled("cuda")


def autocast_narrow_ok(x):
    """QuantizeLinear may ask for the autocast result "rounded once to the operand dtype" only when that dtype IS the
    autocast dtype: F.linear's autocast cast rounds the reference's fp32 result to torch.get_autocast_dtype("cuda"), so
    for an fp16 tensor inside autocast(bf16) (or the reverse) the narrow path would round twice.  Otherwise the callers
    return the fp32 result and let F.linear do the single rounding, exactly as the reference does."""
    return torch.get_autocast_dtype("cuda") == x.dtype


def sym_forward_autocast(x, num_bits, layerwise, wide, lo=-2.0, hi=2.0, train=None):
    """SymQuantizer.forward with autocast arithmetic (fq_sym_fwd_autocast).
    train: None (no side outputs) | "bounds" | "mask".  -> (y, side or bounds or None, rows, cols, got)
    where got is the side information actually produced ("mask", "bounds" or None)."""
    code = _prep(x, "sym_quantize[autocast]")
    rows, cols = rows_cols(tuple(x.shape), layerwise)
    if x.numel() == 0:
        _empty_input("sym_quantize[autocast]", x, layerwise)
        return torch.empty(x.shape, dtype=torch.float32 if wide else x.dtype, device=x.device), None, rows, cols, None
    check_4d(x, layerwise)
    L = _lib.lib()
    xv = rows_view(x, layerwise)
    if xv:   # strided rows: served in the kernel (register-kernel shapes; anything else takes the copy path below)
        mbytes = _mask_bytes(rows, cols, code)
        y, yv = _strided_out(x, torch.float32 if wide else x.dtype)
        if mbytes and yv is not False:
            side = got = None
            bp = mp = None
            if train == "mask":
                side, bp, mp = _side_alloc(rows, mbytes, x.device)
                got = "mask"
            elif train == "bounds":
                side = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
                bp, got = side.data_ptr(), "bounds"
            arr = (_lib.FwdTensorV * 1)(_lib.FwdTensorV(x.data_ptr(), y.data_ptr(), rows, int(num_bits), bp, mp, mbytes if mp else 0, _rv(xv), _rv(yv)))
            rc = _launch(x, L.fq_sym_fwd_multi_v, 1, arr, cols, code, _SEM_AUTOCAST, 2 if wide else 1, float(lo), float(hi))
            if _served(rc, "sym_quantize[autocast]"):
                _view_served()
                return y, side, rows, cols, got
    xc = _contig(x)
    y = torch.empty(xc.shape, dtype=torch.float32 if wide else x.dtype, device=x.device)
    ws_bytes = _ws_bytes(rows, cols, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    ws_ptr = ws.data_ptr() if ws is not None else None
    head = (xc.data_ptr(), y.data_ptr(), rows, cols, int(num_bits), code, _SEM_AUTOCAST, int(wide), float(lo), float(hi))
    what = "sym_quantize[autocast]"
    if train == "mask" and xc is x:  # (a wide result's mask has its own layout: backward = train_backward_wide)
        mbytes = _mask_bytes(rows, cols, code)
        if mbytes:
            side, bp, mp = _side_alloc(rows, mbytes, x.device)
            if _served(_launch(x, L.fq_sym_fwd_autocast, *head, bp, mp, mbytes, ws_ptr, ws_bytes), what):
                return y, side, rows, cols, "mask"   # (xc is x: y has its layout already)
    side = got = bptr = None
    if train in ("mask", "bounds"):
        side = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        bptr, got = side.data_ptr(), "bounds"
    _lib.check(_launch(x, L.fq_sym_fwd_autocast, *head, bptr, None, 0, ws_ptr, ws_bytes), what)
    return _like_input(x, xc, y), side, rows, cols, got


def pair_forward(w, x, w_bits, a_bits, lo, hi, need_w, need_x, wide=False):
    """Two tensors with the same row length in ONE launch (fq_sym_fwd_pair): QuantizeLinear's weight [out, in] (per
    output channel) + input [..., in] (per token), or the attention block's K + V (per token).
    -> (wq, xq, side_w, side_x, rows_w, rows_x, cols) or None when the pair is not served (different dtypes / devices,
    misaligned, non-contiguous, rows too long): use two calls then.
    side_* (row bounds + STE mask, as in train_forward) is produced only for the operands that need a gradient.
    wide: under autocast, return the reference's fp32 results (else those rounded once to the operand dtype)."""
    if w.dtype != x.dtype or w.device != x.device or not w.is_cuda:
        return None
    wv = xv = None
    if not (w.is_contiguous() and x.is_contiguous()):   # strided rows of either operand: served in the kernel where the view allows it
        wv, xv = rows_view(w), rows_view(x)
        if wv is False or xv is False:
            return None
    code = _DTYPES.get(w.dtype)
    if code is None or not (1 <= w.dim() <= 3 and 1 <= x.dim() <= 3) or x.shape[-1] != w.shape[-1] or x.numel() == 0 or w.numel() == 0:
        return None
    cols = w.shape[-1]
    rows_w, rows_x = w.numel() // cols, x.numel() // cols
    mw, mx = _mask_bytes(rows_w, cols, code), _mask_bytes(rows_x, cols, code)
    if not mw or not mx:
        return None
    ac = autocast_active(w)
    wide = bool(wide and ac)
    if ac and not wide and not autocast_narrow_ok(w):
        return None  # autocast dtype != operand dtype: the two-call path returns fp32 results, F.linear rounds once
    L = _lib.lib()
    side_w, bw, pw = _side_alloc(rows_w, mw, w.device) if need_w else _NO_SIDE
    side_x, bx, px = _side_alloc(rows_x, mx, w.device) if need_x else _NO_SIDE
    mw, mx = (mw if need_w else 0), (mx if need_x else 0)
    sem, mode = (_SEM_AUTOCAST, 2 if wide else 1) if ac else (_semantics, 0)
    if wv or xv:
        (wq, wqv), (xq, xqv) = _strided_out(w, torch.float32 if wide else None), _strided_out(x, torch.float32 if wide else None)
        if wqv is False or xqv is False:
            return None
        arr = (_lib.FwdTensorV * 2)(
            _lib.FwdTensorV(w.data_ptr(), wq.data_ptr(), rows_w, w_bits, bw, pw, mw, _rv(wv), _rv(wqv)),
            _lib.FwdTensorV(x.data_ptr(), xq.data_ptr(), rows_x, a_bits, bx, px, mx, _rv(xv), _rv(xqv)))
        if not _served(_launch(w, L.fq_sym_fwd_multi_v, 2, arr, cols, code, sem, mode, lo, hi), "quantize_pair[strided]"):
            return None
        _view_served()
        return wq, xq, side_w, side_x, rows_w, rows_x, cols
    if wide:
        wq, xq = torch.empty(w.shape, dtype=torch.float32, device=w.device), torch.empty(x.shape, dtype=torch.float32, device=w.device)
    else:
        wq, xq = torch.empty_like(w), torch.empty_like(x)
    rc = _launch(w, L.fq_sym_fwd_pair, w.data_ptr(), wq.data_ptr(), rows_w, w_bits, bw, pw, mw,
                 x.data_ptr(), xq.data_ptr(), rows_x, a_bits, bx, px, mx, cols, code, sem, mode, lo, hi)
    if not _served(rc, "quantize_pair"):
        return None
    return wq, xq, side_w, side_x, rows_w, rows_x, cols


# ---- the module's hot path: everything that depends only on (shapes, dtype, device) is decided once per module and shape (`pair_plan`);
# the call itself -- allocate, launch, build the node -- is the C++ node's (csrc/fq_autograd_node.cpp::pair_forward).  Without the node,
# pair_forward / pair_backward above serve (rounds 4-5 had lean Python twins of them here; the C++ node replaced those).
def pair_plan(w, x):
    """-> (code, cols, rows_w, rows_x, mask bytes w, mask bytes x, device index) for a contiguous CUDA weight [out, in] and input [..., in] of
    one dtype that the two-tensor launch serves, else None"""
    if w.dtype != x.dtype or w.device != x.device or not w.is_cuda or w.dim() != 2 or not 1 <= x.dim() <= 3:
        return None
    code = _DTYPES.get(w.dtype)
    cols = w.shape[1]
    if code is None or code == _lib.DTYPE_F64 or x.shape[-1] != cols or not x.numel() or not w.numel():
        return None
    rows_w, rows_x = w.shape[0], x.numel() // cols
    mw, mx = _mask_bytes(rows_w, cols, code), _mask_bytes(rows_x, cols, code)
    if not mw or not mx:
        return None
    return code, cols, rows_w, rows_x, mw, mx, w.device.index


def weight_forward(w, w_bits, lo, hi, need):
    """A QuantizeLinear's weight ALONE (its input was fake-quantized by a sibling projection), shaped like its half of pair_forward:
    -> (wq, side or None, rows, cols), or None where the pair would not be served either (the caller then takes the ordinary node).
    Under autocast: the reference's arithmetic rounded once to the operand dtype (the narrow form), as in the pair launch."""
    if not (w.is_cuda and w.is_contiguous() and w.dim() == 2 and w.numel()):
        return None
    if autocast_active(w):
        if not autocast_narrow_ok(w):
            return None
        y, side, rows, cols, got = sym_forward_autocast(w, w_bits, False, wide=False, lo=lo, hi=hi, train="mask" if need else None)
        if need and got != "mask":
            return None
        return y, (side if need else None), rows, cols
    if need:
        return train_forward("sym", w, w_bits, False, lo, hi)
    return sym_quantize(w, w_bits), None, w.shape[0], w.shape[1]


def pair_backward(gw, gx, side_w, side_x, rows_w, rows_x, cols, lo, hi, inplace_w=False):
    """STE backward of both operands in one launch; either gradient may be None (then only the other is computed).
    inplace_w: the first tensor's gradient (a weight's) is masked where it stands and returned itself (see train_backward)."""
    if gw is None or gx is None:
        if gx is None:
            return train_backward(gw, side_w, rows_w, cols, lo, hi, inplace=inplace_w), None
        return None, train_backward(gx, side_x, rows_x, cols, lo, hi)
    code = _DTYPES.get(gw.dtype)
    if not (gw.is_contiguous() and gx.is_contiguous()):   # strided rows: masked in the kernel
        res = _mask_backward_v([gw, gx], [side_w, side_x], [rows_w, rows_x], cols, lo, hi, code, False, [inplace_w, False])
        if res is not None:
            return res[0], res[1]
    gw, ow, slot_w = _mask_slot(gw, side_w, rows_w, inplace_w)
    gx, ox, slot_x = _mask_slot(gx, side_x, rows_x)
    rc = _launch(gw, _lib.lib().fq_ste_bwd_mask_pair, *slot_w, *slot_x, cols, lo, hi, code)
    if not _served(rc, "quantize_linear_pair_backward"):
        return train_backward(gw, side_w, rows_w, cols, lo, hi, inplace=inplace_w), train_backward(gx, side_x, rows_x, cols, lo, hi)
    return ow, ox


def pair_backward_wide(gw, gx, side_w, side_x, rows_w, rows_x, cols, lo, hi, out_dtype):
    """pair_backward behind a wide (fp32-result) pair_forward: fp32 gradients in, gradients in the operands' dtype out."""
    if gw is None or gx is None:
        if gx is None:
            return train_backward_wide(gw, side_w, rows_w, cols, lo, hi, out_dtype), None
        return None, train_backward_wide(gx, side_x, rows_x, cols, lo, hi, out_dtype)
    code = _DTYPES.get(out_dtype)
    gw, ow, slot_w = _mask_slot(gw, side_w, rows_w, False, out_dtype)
    gx, ox, slot_x = _mask_slot(gx, side_x, rows_x, False, out_dtype)
    rc = _launch(gw, _lib.lib().fq_ste_bwd_mask_wide, *slot_w, *slot_x, cols, float(lo), float(hi), code)
    _lib.check(rc, "quantize_pair_backward_wide")
    return ow, ox


def multi_forward(tensors, bits, need, lo, hi):
    """2..4 tensors with the same row length, dtype and device in ONE launch (fq_sym_fwd_multi): a QuantizeLinear's weight
    and input plus the weights of the sibling projections that share that input (q/k/v, gate/up).
    tensors / bits / need: parallel lists (need[i]: record bounds + STE mask for tensor i's backward).
    -> ([y_i], [side_i or None], [rows_i], cols) or None when the group is not served."""
    n = len(tensors)
    t0 = tensors[0]
    if not 2 <= n <= _lib.MAX_TENSORS or not t0.is_cuda:
        return None
    code = _DTYPES.get(t0.dtype)
    cols = t0.shape[-1]
    if code is None:
        return None
    rows, mbytes = [], []
    for t in tensors:
        if t.dtype != t0.dtype or t.device != t0.device or not t.is_contiguous() or not 1 <= t.dim() <= 3 or t.shape[-1] != cols or t.numel() == 0:
            return None
        r = t.numel() // cols
        mb = _mask_bytes(r, cols, code)
        if not mb:
            return None
        rows.append(r)
        mbytes.append(mb)
    ac = autocast_active(t0)
    if ac and not autocast_narrow_ok(t0):
        return None
    ys = [torch.empty_like(t) for t in tensors]
    sides = []
    arr = (_lib.FwdTensor * n)()
    for i, (t, y) in enumerate(zip(tensors, ys)):
        sd, bp, mp = _side_alloc(rows[i], mbytes[i], t0.device) if need[i] else _NO_SIDE
        sides.append(sd)
        arr[i] = _lib.FwdTensor(t.data_ptr(), y.data_ptr(), rows[i], int(bits[i]), bp, mp, mbytes[i] if need[i] else 0)
    rc = _launch(t0, _lib.lib().fq_sym_fwd_multi, n, arr, cols, code, _SEM_AUTOCAST if ac else _semantics, 1 if ac else 0, float(lo), float(hi))
    if not _served(rc, "quantize_multi"):
        return None
    return ys, sides, rows, cols


def multi_backward(grads, sides, rows, cols, lo, hi, inplace=None):
    """STE backward of the tensors of a multi_forward in one launch; grads[i] may be None (that tensor is skipped).
    inplace[i]: tensor i's gradient is masked where it stands and returned itself (weights; see train_backward)."""
    live = [i for i, g in enumerate(grads) if g is not None]
    out = [None] * len(grads)
    inplace = inplace or [False] * len(grads)
    if not live:
        return out
    if len(live) == 1:
        i = live[0]
        out[i] = train_backward(grads[i], sides[i], rows[i], cols, lo, hi, inplace=inplace[i])
        return out
    code = _DTYPES.get(grads[live[0]].dtype)
    gs = {}
    arr = (_lib.BwdTensor * len(live))()
    for j, i in enumerate(live):
        gs[i], out[i], slot = _mask_slot(grads[i], sides[i], rows[i], inplace[i])
        arr[j] = _lib.BwdTensor(*slot)
    rc = _launch(gs[live[0]], _lib.lib().fq_ste_bwd_mask_multi, len(live), arr, cols, float(lo), float(hi), code, 0)
    if not _served(rc, "quantize_multi_backward"):
        for i in live:
            out[i] = train_backward(gs[i], sides[i], rows[i], cols, lo, hi, inplace=inplace[i])
    return out


def quantize_train(kind, x, num_bits, layerwise, lo, hi, group_size=None):
    """Training-mode forward (fq_*_fwd_train): -> (y, row_bounds, mask) or None if this shape/alignment is
    not served by the STE-mask path (the caller then uses the general forward + x-based backward).
    Convenience form of train_forward() with the side buffer split into its two views.
    group_size: group-wise scales (fq_group_fwd); the bounds and the mask keep the full-row layout, so ste_backward_mask serves them."""
    if group_size is not None:
        g = check_group(tuple(x.shape), group_size, layerwise)
        _prep(x, f"{kind}_quantize")
        res = group_forward(kind, x, num_bits, g, lo=float(lo), hi=float(hi), train=True)
    else:
        res = train_forward(kind, x, num_bits, layerwise, float(lo), float(hi))
    if res is None:
        return None
    y, side, rows, _ = res
    return (y,) + split_side(side, rows)


def ste_backward_mask(grad_output, lo, hi, row_bounds, mask, rows, cols, inplace=False):
    """STE backward from the (row_bounds, mask) a quantize_train call recorded -- x is not needed."""
    code = _prep(grad_output, "ste_backward_mask")
    g = _aligned(grad_output)  # a contiguous gradient can still be an offset view into a flat buffer
    gx = g if inplace else torch.empty_like(g)
    if g.numel() == 0:
        return gx
    rc = _launch(g, _lib.lib().fq_ste_bwd_mask, g.data_ptr(), gx.data_ptr(), rows, cols, float(lo), float(hi), row_bounds.data_ptr(),
                 mask.data_ptr(), mask.numel(), code)
    _lib.check(rc, "ste_backward_mask")
    return gx


def low_bit_weight(w, scale, w_bits):
    """Elementwise part of QuantizeLinear's 1-/2-bit weight branch (utils_quant.py:203-242), forward value of
    `q.detach() - w.detach() + w`.  `scale`: [rows, 1] / [rows] per-row or 0-dim layerwise, same dtype as w."""
    code = _prep(w, "low_bit_weight")
    if w.dim() != 2:
        raise ValueError("low_bit_weight expects a 2-D weight")
    wc = _contig(w)
    sc = scale.to(w.dtype).contiguous()
    per_row = 1 if sc.numel() == w.shape[0] and sc.numel() != 1 else 0
    if not per_row and sc.numel() != 1:
        raise ValueError(f"scale has {sc.numel()} elements for a weight with {w.shape[0]} rows")
    out = torch.empty_like(wc)
    if wc.numel():
        rc = _launch(w, _lib.lib().fq_w12_fwd, wc.data_ptr(), sc.data_ptr(), out.data_ptr(), wc.shape[0], wc.shape[1], int(w_bits), per_row, code)
        _lib.check(rc, "low_bit_weight")
    return out


def low_bit_weight_fused(w, w_bits):
    """The 1-/2-bit branch in ONE launch, per-row mean|w| reduced inside the kernel in ATen's own summation order (fq_w12_fwd_rows):
    bit-identical to `abs().mean(dim=1)` + the elementwise chain on this device.  -> (out, scale[rows]) or None when the shape is not
    served (the caller then takes ATen's reduction + fq_w12_fwd)."""
    code = _prep(w, "low_bit_weight_fused")
    if code == _lib.DTYPE_F64 or w.dim() != 2 or not w.is_contiguous() or w.numel() == 0:
        return None
    out = torch.empty_like(w)
    scale = torch.empty(w.shape[0], dtype=w.dtype, device=w.device)
    rc = _launch(w, _lib.lib().fq_w12_fwd_rows, w.data_ptr(), out.data_ptr(), scale.data_ptr(), w.shape[0], w.shape[1], int(w_bits), code)
    if not _served(rc, "low_bit_weight_fused"):
        return None
    return out, scale


# ---- group-wise scales: every run of `group_size` consecutive elements of a row has its own scale ------------------------------------
# y = Q(x.reshape(-1, g)).reshape(x.shape), in the arithmetic the row-wise path uses for that tensor.  Where fq_group_fwd serves the shape
# (contiguous 16-byte aligned bf16 / fp16 / fp32, groups of 4..64 16-byte vectors -- bf16 / fp16 g = 32, 64, 128, 256, 512; fp32 g = 16, 32,
# 64, 128, 256 --, rows that fit the register kernels) it runs one launch
# with the side outputs of the FULL row; everything else takes the row-wise kernels on the [rows * C / g, g] view (same values).  Which of
# the two ran is counted here (utils_quant.stats() reports it): the route follows from the inputs alone.
group_counts = {"group_launch": 0, "group_view_route": 0}


def check_group(shape, group_size, layerwise=False):
    """-> g as an int after the argument checks of the group-wise API (ValueError for what is not defined)"""
    if isinstance(group_size, (bool, str)) or isinstance(group_size, torch.Tensor):
        raise ValueError(f"group_size must be a positive integer, got {group_size!r}")
    if not isinstance(group_size, int):
        try:
            g = int(group_size)
        except (TypeError, ValueError):
            raise ValueError(f"group_size must be a positive integer, got {group_size!r}") from None
        if g != group_size:
            raise ValueError(f"group_size must be a positive integer, got {group_size!r}")
    else:
        g = group_size
    if layerwise:
        raise ValueError("group_size cannot be combined with layerwise=True")
    if len(shape) > 3:
        raise ValueError(f"group-wise fake quantization takes tensors of at most 3 dimensions, got {len(shape)}")
    if g <= 0:
        raise ValueError(f"group_size must be positive, got {g}")
    cols = shape[-1] if len(shape) else 1
    if cols % g:
        raise ValueError(f"group_size={g} does not divide the last dimension ({cols})")
    return g


def group_forward(kind, x, num_bits, group_size, autocast=False, lo=-2.0, hi=2.0, train=False):
    """fq_group_fwd -> (y, side, rows, cols) or None when the kernel does not serve this tensor (the caller takes the view route).
    side: None, or (train=True) one uint8 buffer of float[rows][2] full-row bounds followed by the row bitmap, as train_forward's."""
    code = _DTYPES.get(x.dtype)
    if code is None or code == _lib.DTYPE_F64 or not x.is_cuda or not x.is_contiguous() or x.numel() == 0 or x.data_ptr() & 15:
        return None
    rows, cols = rows_cols(tuple(x.shape), False)
    side, bp, mp = _NO_SIDE
    mbytes = 0
    if train:
        mbytes = _mask_bytes(rows, cols, code)
        if not mbytes:
            return None
        side, bp, mp = _side_alloc(rows, mbytes, x.device)
    y = torch.empty_like(x)
    rc = _launch(x, _lib.lib().fq_group_fwd, 1 if kind == "asym" else 0, x.data_ptr(), y.data_ptr(), rows, cols, int(group_size), int(num_bits), code,
                 _SEM_AUTOCAST if autocast else _semantics, 1 if autocast else 0, float(lo), float(hi), bp, mp, mbytes)
    if not _served(rc, f"{kind}_quantize[group]"):
        return None
    group_counts["group_launch"] += 1
    return y, side, rows, cols


def group_view(x, group_size):
    """the [rows * C / g, g] view the row-wise path quantizes for the view route (a copy where x's layout has no such view)"""
    return x.reshape(-1, group_size)


def _grouped(kind, x, num_bits, group_size, want_bounds):
    g = check_group(tuple(x.shape), group_size)
    code = _prep(x, f"{kind}_quantize")
    res = group_forward(kind, x, num_bits, g, lo=-2.0, hi=2.0, train=False) if not want_bounds else None
    if res is None and want_bounds:
        res = group_forward(kind, x, num_bits, g, lo=-2.0, hi=2.0, train=True)
    if res is not None:
        y, side, rows, _ = res
        return (y, split_side(side, rows)[0]) if want_bounds else y
    group_counts["group_view_route"] += 1
    if x.numel() == 0:
        return (torch.empty_like(x), None) if want_bounds else torch.empty_like(x)
    yv, bv, _, _ = _rowwise(kind, group_view(x, g), num_bits, False, want_bounds and code != _lib.DTYPE_F64, False)
    y = yv.reshape(x.shape)
    if not want_bounds:
        return y
    if bv is None:
        return y, None
    rows, _ = rows_cols(tuple(x.shape), False)
    b = bv.view(rows, -1, 2)   # per-group bounds -> the row's (max / min propagate NaN, as the kernels' bounds do)
    return y, torch.stack((b[..., 0].amax(1), b[..., 1].amin(1)), 1)


def sym_quantize(x, num_bits, layerwise=False, want_bounds=False, group_size=None):
    """SymQuantizer.forward (utils_quant.py:37-74).  -> y, or (y, row_bounds) if want_bounds.
    group_size: one scale per `group_size` consecutive elements of a row (the forward of the [-1, group_size] view); row_bounds are
    still those of the whole row."""
    if group_size is not None:
        return _grouped("sym", x, num_bits, group_size, want_bounds)
    y, bounds, _, _ = _rowwise("sym", x, num_bits, layerwise, want_bounds, False)
    return (y, bounds) if want_bounds else y


def asym_quantize(x, num_bits, layerwise=False, want_bounds=False, group_size=None):
    """AsymQuantizer.forward (utils_quant.py:96-149).  group_size: as sym_quantize."""
    if group_size is not None:
        return _grouped("asym", x, num_bits, group_size, want_bounds)
    y, bounds, _, _ = _rowwise("asym", x, num_bits, layerwise, want_bounds, False)
    return (y, bounds) if want_bounds else y


def sym_quantize_debug(x, num_bits, layerwise=False):
    """-> (y, idx int32, s float32[rows]) -- the bin indices the parity tests compare bit-exactly."""
    y, _, idx, scale = _rowwise("sym", x, num_bits, layerwise, False, True)
    return y, idx, scale


def asym_quantize_debug(x, num_bits, layerwise=False):
    """-> (y, idx int32, {alpha, beta} float32[rows, 2])"""
    y, _, idx, scale = _rowwise("asym", x, num_bits, layerwise, False, True)
    return y, idx, scale


def ste_backward(grad_output, x, lo, hi, row_bounds=None, rows_cols_hint=None):
    """STE mask (utils_quant.py:83-87): grad where lo < x < hi (or x is NaN), else 0."""
    code = _prep(x, "ste_backward")
    if grad_output.device != x.device:
        raise RuntimeError("ste_backward: grad_output and input live on different devices")
    if grad_output.shape != x.shape:
        raise RuntimeError(f"ste_backward: shape mismatch {tuple(grad_output.shape)} vs {tuple(x.shape)}")
    if grad_output.dtype != x.dtype:  # cannot happen through the autograd Functions (output dtype == input dtype)
        raise NotImplementedError(f"ste_backward: grad dtype {grad_output.dtype} != input dtype {x.dtype}")
    L = _lib.lib()
    if not (grad_output.is_contiguous() and x.is_contiguous()) and grad_output.numel() and code != _lib.DTYPE_F64:
        gv, xv = rows_view(grad_output), rows_view(x)   # strided rows of the gradient and / or the saved input: served in the kernel
        if gv is not False and xv is not False:
            gx, ov = _strided_out(grad_output)
            if ov is not False:
                rows, cols = rows_cols(tuple(x.shape), False)
                rc = _launch(x, L.fq_ste_bwd_v, grad_output.data_ptr(), _rv(gv), x.data_ptr(), _rv(xv), gx.data_ptr(), _rv(ov), rows, cols,
                             float(lo), float(hi), None, code)
                if _served(rc, "ste_backward[strided]"):
                    _view_served()
                    return gx
    g, xc = _contig(grad_output), _contig(x)
    gx = torch.empty_like(g)
    if g.numel() == 0:
        return gx
    if row_bounds is not None:
        rows, cols = rows_cols_hint
        rc = _launch(x, L.fq_ste_bwd_rows, g.data_ptr(), xc.data_ptr(), gx.data_ptr(), rows, cols, float(lo), float(hi), row_bounds.data_ptr(), code)
    else:
        rc = _launch(x, L.fq_ste_bwd, g.data_ptr(), xc.data_ptr(), gx.data_ptr(), g.numel(), float(lo), float(hi), code)
    _lib.check(rc, "ste_backward")
    return gx


# ---- the integer side of the forward: packed bins + scales for export, scale pre-pass --------------------
_CONTAINERS = {"int4": _lib.BINS_INT4, "int8": _lib.BINS_INT8, "int16": _lib.BINS_INT16}


class QuantExport:
    """Result of sym_export / asym_export.
      bins      packed integer bins: int8 / int16 tensor of the input's shape, or (int4) uint8 [rows, ceil(cols/2)] with
                element 2k in the low nibble of byte k
      scales    float32 [rows, 2]: Sym {s, t2 = s + 1e-6};  Asym {a = alpha + 1e-8, beta}
      overflow  int32 [rows]: elements the container saturated (0 everywhere <=> dequantize() == the fake-quant forward)
    group_size None (one scale per row), or g: scales are float32 [rows, cols / g, 2] and overflow int32 [rows, cols / g], one entry per
                group; int4 bins of an even g are byte for byte the row-major packing of the full rows ([rows, cols / 2])
    """
    __slots__ = ("kind", "bins", "scales", "overflow", "container", "num_bits", "shape", "rows", "cols", "dtype", "group_size")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def unpacked(self):
        """bins as an int32 tensor [rows, cols]"""
        b = self.bins
        if self.container != "int4":
            v = b.reshape(self.rows, self.cols).to(torch.int32)
            return v & 0xFFFF if (self.kind == "asym" and self.container == "int16") else v   # unsigned 16-bit bins
        g = getattr(self, "group_size", None)
        prow, pcols = (self.rows, self.cols) if g is None else (self.rows * (self.cols // g), g)   # rows as packed: the group view's
        lo, hi = (b & 0xF).to(torch.int32), (b >> 4).to(torch.int32)
        v = torch.stack((lo, hi), dim=-1).reshape(prow, -1)[:, :pcols].reshape(self.rows, self.cols)
        return torch.where(v >= 8, v - 16, v) if self.kind == "sym" else v

    def dequantize(self):
        """the fake-quant forward's value, recomputed from bins + scales with the reference's op order (fp32 tensors ->
        round to the tensor dtype after every op); bit-identical to SymQuantizer / AsymQuantizer.forward on rows with
        overflow == 0 (cpu_eager semantics: true divisions)."""
        q = self.unpacked().to(torch.float32)
        sc = self.scales
        dt = self.dtype
        g = getattr(self, "group_size", None)
        if g is not None:   # one scale per group: the row-wise formula on the [rows * cols / g, g] view
            q = q.reshape(-1, g)
            sc = sc.reshape(-1, 2)
        if self.kind == "sym":
            y = (q / sc[:, 1:2]).to(dt)
        else:
            S = torch.tensor(float(2 ** self.num_bits - 1), device=q.device)  # a tensor divisor: true division (a Python scalar
            y = (q / S).to(dt).to(torch.float32)                               # would become a multiply by 1/S on the GPU)
            y = (y * sc[:, 0:1]).to(dt).to(torch.float32)
            y = (y + sc[:, 1:2]).to(dt)
        return y.reshape(self.shape)


def default_container(kind, num_bits, dtype):
    """smallest container that is lossless for every input: Sym bins reach +-(qmax + 1) in bf16 at 8 bits (no clamp in
    the reference), so 8-bit bf16 defaults to int16; ask for "int8" explicitly to get the saturating deployment format."""
    if kind == "asym":
        return "int4" if num_bits <= 4 else "int8" if num_bits <= 8 else "int16"
    if num_bits <= 4:
        return "int4"
    if num_bits <= 7 or (num_bits == 8 and dtype != torch.bfloat16):
        return "int8"
    return "int16"


def _export_grouped(kind, x, num_bits, group_size, container, autocast):
    """the export kernels on the [rows * C / g, g] view (no kernel of its own), reshaped to the full tensor's rows"""
    g = check_group(tuple(x.shape), group_size)
    _prep(x, f"{kind}_export")
    e = _export(kind, group_view(x, g), num_bits, False, container, autocast)
    rows, cols = rows_cols(tuple(x.shape), False)
    bins = e.bins
    if e.container != "int4":
        bins = bins.reshape(x.shape)
    elif g % 2 == 0:
        bins = bins.reshape(rows, cols // 2)
    return QuantExport(kind=kind, bins=bins, scales=e.scales.view(rows, cols // g, 2), overflow=e.overflow.view(rows, cols // g),
                       container=e.container, num_bits=e.num_bits, shape=tuple(x.shape), rows=rows, cols=cols, dtype=x.dtype, group_size=g)


def _export(kind, x, num_bits, layerwise, container, autocast):
    what = f"{kind}_export"
    code = _prep(x, what)
    rows, cols = rows_cols(tuple(x.shape), layerwise)
    if x.numel() == 0:
        raise RuntimeError(f"{what}: empty tensor")
    container = container or default_container(kind, num_bits, x.dtype)
    cc = _CONTAINERS.get(container)
    if cc is None:
        raise ValueError(f"{what}: container must be one of {sorted(_CONTAINERS)}, got {container!r}")
    xc = _contig(x)
    L = _lib.lib()
    nbytes = L.fq_export_bins_bytes(rows, cols, cc)
    raw = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    scales = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    overflow = torch.empty(rows, dtype=torch.int32, device=x.device)
    head = (xc.data_ptr(), raw.data_ptr(), scales.data_ptr(), overflow.data_ptr(), rows, cols, int(num_bits), cc, code)
    if kind == "sym":
        rc = _launch(x, L.fq_sym_export, *head, _SEM_AUTOCAST if autocast else _semantics, 1 if autocast else 0)
    else:
        rc = _launch(x, L.fq_asym_export, *head, _semantics)
    _lib.check(rc, what)
    if container == "int8":
        bins = (raw.view(torch.int8) if kind == "sym" else raw).view(xc.shape)
    elif container == "int16":
        bins = raw.view(torch.int16).view(xc.shape)   # Asym 16-bit bins 32768..65535 read as negative int16: use unpacked()
    else:
        bins = raw.view(rows, (cols + 1) // 2)
    return QuantExport(kind=kind, bins=bins, scales=scales, overflow=overflow, container=container, num_bits=int(num_bits),
                       shape=tuple(xc.shape), rows=rows, cols=cols, dtype=x.dtype, group_size=None)


def sym_export(x, num_bits, layerwise=False, container=None, autocast=None, group_size=None):
    """SymQuantizer's integer bins `torch.round(input * s)` (utils_quant.py:71-72) packed into int4 / int8 / int16 + per-row
    {s, t2}.  autocast: None = follow torch.is_autocast_enabled (as the forward does), or force True / False.
    group_size: {s, t2} per group of `group_size` elements (see QuantExport)."""
    ac = autocast_active(x) if autocast is None else bool(autocast)
    if group_size is not None:
        if layerwise:
            check_group(tuple(x.shape), group_size, layerwise)
        return _export_grouped("sym", x, num_bits, group_size, container, ac)
    return _export("sym", x, num_bits, layerwise, container, ac)


def asym_export(x, num_bits, layerwise=False, container=None, group_size=None):
    """AsymQuantizer's bins `torch.round(input_normalized * s)` (utils_quant.py:144-146), unsigned, + per-row {alpha+1e-8, beta}
    group_size: {alpha+1e-8, beta} per group of `group_size` elements (see QuantExport)."""
    if group_size is not None:
        if layerwise:
            check_group(tuple(x.shape), group_size, layerwise)
        return _export_grouped("asym", x, num_bits, group_size, container, False)
    return _export("asym", x, num_bits, layerwise, container, False)


def sym_row_scales(x, num_bits, layerwise=False, autocast=None):
    """per-row {s, t2} of SymQuantizer.forward without the elementwise pass (fq_sym_row_scales) -> float32 [rows, 2]"""
    code = _prep(x, "sym_row_scales")
    rows, cols = rows_cols(tuple(x.shape), layerwise)
    if x.numel() == 0:
        raise RuntimeError("sym_row_scales: empty tensor")
    ac = autocast_active(x) if autocast is None else bool(autocast)
    xc = _contig(x)
    scales = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    rc = _launch(x, _lib.lib().fq_sym_row_scales, xc.data_ptr(), scales.data_ptr(), rows, cols, int(num_bits), code, _SEM_AUTOCAST if ac else _semantics,
                 1 if ac else 0, -2.0, 2.0, None, None, 0)
    _lib.check(rc, "sym_row_scales")
    return scales


# ---- OCP Microscaling (MX) block scales: 32 consecutive elements of the last dimension share one E8M0 power-of-two scale ----------------
# (include/llmqat_fakequant.h "MX block scales").  One launch per tensor; a non-contiguous or misaligned input takes one
# .contiguous() copy first (a correctness path, counted as mx_copy_route).  No CPU implementation: CPU tensors raise.
MX_FORMATS = {"mxfp4": _lib.MX_FP4_E2M1, "mxfp6_e2m3": _lib.MX_FP6_E2M3, "mxfp6_e3m2": _lib.MX_FP6_E3M2,
              "mxfp8_e4m3": _lib.MX_FP8_E4M3, "mxfp8_e5m2": _lib.MX_FP8_E5M2}
MX_BLOCK = 32
# rotate=True: the same launches quantize x R, R block-diagonal along the last dimension with blocks H64 / 8 (the
# 64 x 64 Sylvester Hadamard matrix, normalised: orthonormal, symmetric, its own inverse).  Rotating both operands of a product along K
# leaves the product unchanged and spreads an outlier over its 64-element run before the block scales are taken.
MX_ROTATE = 64
# scale_rule: "floor" is OCP's E = floor(log2 amax) - emax, under which the top binade of a block may saturate;
# "ceil" is the smallest E with amax * 2^-E <= max-normal, under which nothing does.  The saturation mask (return_mask) has one bit per
# element, bit i & 7 of byte i >> 3 for flat element i, 0 where saturation changed the rounded value; mx_ste_backward applies it.
MX_SCALE_RULES = ("floor", "ceil")
# mx_quantize_sr: the same two launches with stochastic rounding onto the element grid -- each element goes to one of its
# two grid neighbours with the probabilities that make the result unbiased -- for the gradient operand of the backward GEMMs.  The noise is
# Philox4x32-10 on (seed, stream, flat element index), computed inside the kernels (fqs_mx_fwd / fqs_mx_fwd_cols of the third header).
mx_counts = {"mx_launch": 0, "mx_export_launch": 0, "mx_copy_route": 0, "mx_gemm_launch": 0, "mx_gemm_skinny": 0, "mx_gemm_tiled": 0,
             "mx_rotate_launch": 0, "mx_mask_launch": 0, "mx_ste_launch": 0, "mx_cols_launch": 0, "mx_sr_launch": 0, "mx_sr_cols_launch": 0,
             "mx_dequant_launch": 0}


def _mx_format(fmt):
    """-> the C code of an MX format name; ValueError for anything else"""
    code = MX_FORMATS.get(fmt) if isinstance(fmt, str) else None
    if code is None:
        raise ValueError(f"unknown MX format {fmt!r}: one of {', '.join(MX_FORMATS)}")
    return code


def check_mx(shape, fmt):
    """-> the format's C code after the argument checks of the MX API (ValueError for an unknown format or a last dimension that is not a
    multiple of 32)"""
    code = _mx_format(fmt)
    if len(shape) == 0:
        raise ValueError("MX formats take tensors with at least one dimension")
    if shape[-1] % MX_BLOCK:
        raise ValueError(f"MX formats need a last dimension that is a multiple of {MX_BLOCK}, got {shape[-1]}")
    return code


def check_mx_rotate(shape, what="mx_rotate"):
    """The shape check of every rotated MX call: ValueError unless the last dimension is a multiple of 64."""
    if len(shape) == 0:
        raise ValueError(f"{what}: the rotation takes tensors with at least one dimension")
    if shape[-1] % MX_ROTATE:
        raise ValueError(f"{what}: the block-Hadamard rotation needs a last dimension that is a multiple of {MX_ROTATE}, got {shape[-1]}")


def check_mx_scale_rule(scale_rule, what="mx_quantize"):
    """-> FQ_MX_FLAG_CEIL or 0; ValueError for anything but "floor" / "ceil"."""
    if not isinstance(scale_rule, str) or scale_rule not in MX_SCALE_RULES:
        raise ValueError(f"{what}: unknown scale_rule {scale_rule!r}: one of {', '.join(MX_SCALE_RULES)}")
    return _lib.MX_FLAG_CEIL if scale_rule == "ceil" else 0


def check_mx_axis(ndim, axis, what="mx_quantize"):
    """-> -1 or -2, the axis the MX blocks run along; ValueError for anything but the last two axes (negative or not) of the tensor"""
    if isinstance(axis, int) and not isinstance(axis, bool):
        if axis in (-1, ndim - 1):
            return -1
        if axis in (-2, ndim - 2) and ndim >= 2:
            return -2
        if axis == -2:
            raise ValueError(f"{what}: axis=-2 needs a tensor with at least two dimensions, got {ndim}")
    raise ValueError(f"{what}: axis={axis!r}: MX blocks run along the last axis (-1) or the one before it (-2)")


def check_mx_cols(shape, fmt, what="mx_quantize"):
    """-> the format's C code after the argument checks of the column axis: at least two dimensions, shape[-2] a multiple of 32 (the last
    dimension is free)"""
    code = _mx_format(fmt)
    if len(shape) < 2:
        raise ValueError(f"{what}: axis=-2 needs a tensor with at least two dimensions, got {len(shape)}")
    if shape[-2] % MX_BLOCK:
        raise ValueError(f"{what}: axis=-2 needs a second-to-last dimension that is a multiple of {MX_BLOCK}, got {shape[-2]}")
    return code


def _mx_aligned(t, count):
    """t where it is contiguous and 16-byte aligned, else one fresh copy (aligned as every allocation); count: as an mx_copy_route"""
    if t.is_contiguous() and not t.data_ptr() & 15:
        return t
    if count:
        mx_counts["mx_copy_route"] += 1
    return t.clone() if t.is_contiguous() else t.contiguous()


def _mx_input(x, fmt, what, rotate=False, axis=-1, as_given=False):
    """The input checks of every MX launch, in their order: format (None: the call has none) and shape for `axis`, the rotation's shape,
    type / device / dtype, then the copy route -> (tensor to launch on, format code, dtype code, the axis its blocks run along).  The
    column kernel takes a contiguous, aligned tensor of whole 16-byte rows: any other comes back transposed, for the row kernel (-1).
    as_given (the stochastic forms, whose noise is indexed on the tensor as it is given): nothing is transposed -- along -2 a last dimension
    that is not whole 16-byte vectors is refused, and a non-contiguous or misaligned input takes the one copy of the last axis."""
    code = None
    if isinstance(x, torch.Tensor):
        if axis == -2:
            code = check_mx_cols(tuple(x.shape), fmt, what)
            if as_given and (x.shape[-1] * x.element_size()) % 16:
                raise ValueError(f"{what}: axis=-2 needs a last dimension of whole 16-byte vectors ({16 // x.element_size()} elements of {x.dtype}), "
                                 f"got {x.shape[-1]}: the noise is indexed on the tensor as given, so the transposed route does not serve it")
        elif fmt is not None:
            code = check_mx(tuple(x.shape), fmt)
        if rotate:
            check_mx_rotate(tuple(x.shape), what)
    dt = _prep(x, what)
    if dt == _lib.DTYPE_F64:
        raise NotImplementedError(f"{what}: float64 is not served by the MX formats (float32, bfloat16, float16 are)")
    if axis == -2 and not as_given and (not x.is_contiguous() or x.data_ptr() & 15 or (x.shape[-1] * x.element_size()) % 16):
        mx_counts["mx_copy_route"] += 1
        x, axis = x.transpose(-1, -2).contiguous(), -1
    return _mx_aligned(x, True), code, dt, axis


def _mx_launch(what, entry, counter, t, head, *tail, dims=None):
    """The tail of every MX launch: lib.<entry>(*head, *dims, *tail, stream) on t's device, the status checked under the caller's name,
    mx_counts[counter] bumped; dims None: t's (rows, cols).  A dimension of 0: nothing is launched or counted.  -> whether it launched."""
    if dims is None:
        cols = t.shape[-1]
        dims = (t.numel() // cols if cols else 0, cols)
    if 0 in dims:
        return False
    _lib.check(_launch(t, getattr(_lib.lib(), entry), *head, *dims, *tail), what)
    mx_counts[counter] += 1
    return True


def mx_rotate(x):
    """x R (same shape and dtype): every run of 64 elements along the last dimension times H64 / 8, in fp32, rounded once to x's dtype.
    R is its own inverse and its own transpose, so this is also the backward of itself.  One launch (fq_block_rotate)."""
    x, _, dt, _ = _mx_input(x, None, "mx_rotate", True)
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    _mx_launch("mx_rotate", "fq_block_rotate", "mx_rotate_launch", x, (x.data_ptr(), y.data_ptr()), dt)
    return y


def _mx_quantize(x, fmt, rotate, scale_rule, return_mask, axis):
    """mx_quantize / mx_quantize_axis: one launch of the row kernel (fq_mx_fwd_ex), or along axis -2 one of the
    column kernel (fqt_mx_fwd_cols) where it takes the input, else the row kernel on the transposed copy, transposed back."""
    down = axis != -1 and isinstance(x, torch.Tensor) and check_mx_axis(x.dim(), axis) == -2
    if down and (rotate or return_mask):
        raise ValueError(f"mx_quantize: the column axis (axis=-2) does not serve {'rotate' if rotate else 'return_mask'}=True yet")
    flags = check_mx_scale_rule(scale_rule) | (_lib.MX_FLAG_ROTATE if rotate else 0)
    x, code, dt, axis = _mx_input(x, fmt, "mx_quantize", rotate, -2 if down else -1)
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    if axis == -2:
        _mx_launch("mx_quantize", "fqt_mx_fwd_cols", "mx_cols_launch", x, (x.data_ptr(), y.data_ptr()), code, dt, flags)
        return y
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) if return_mask else None
    head = (x.data_ptr(), y.data_ptr(), mask.data_ptr() if return_mask else None)
    if _mx_launch("mx_quantize", "fq_mx_fwd_ex", "mx_launch", x, head, code, dt, flags) and return_mask:
        mx_counts["mx_mask_launch"] += 1
    if down:
        return y.transpose(-1, -2).contiguous()
    return (y, mask) if return_mask else y


def mx_quantize_axis(x, fmt, rotate=False, scale_rule="floor", return_mask=False, axis=-1):
    """mx_quantize with a choice of the axis the blocks run along: -1 (or ndim - 1) is mx_quantize itself; -2 (or ndim - 2): the blocks run
    down the columns -- 32 consecutive elements of the second-to-last dimension (a multiple of 32; the last one is free) share a scale;
    the result is contiguous and equals the last-axis result of the transposed tensor, transposed back, bit for bit.  One launch of its
    own kernel; the rotation and the mask are not served there (ValueError).  (mx_quantize's body, _mx_quantize, under a name that takes
    the axis: mx_quantize's own parameter list is pinned by tests/test_mx_rules_cpu.py.)"""
    return _mx_quantize(x, fmt, rotate, scale_rule, return_mask, axis)


def mx_quantize(x, fmt, rotate=False, scale_rule="floor", return_mask=False):
    """MX fake quantization of x (same shape and dtype): each block of 32 elements along the last dimension scaled by its shared power
    of two, rounded onto the element grid of `fmt` and saturated, then scaled back and rounded once to x's dtype.  rotate=True: of the
    fp32 values of x R (mx_rotate) instead, in the same single launch; the result is in the rotated basis.
    scale_rule="ceil": the shared exponent under which no element of a finite block saturates.  return_mask=True -> (y, mask): mask is a
    uint8 tensor of numel / 8 bytes written by the same launch, a 0 bit where saturation changed the element (of x R under rotate)."""
    return _mx_quantize(x, fmt, rotate, scale_rule, return_mask, -1)


def check_mx_sr_word(value, name, what="mx_quantize_sr"):
    """-> value, a Python int in [0, 2^64) (a seed or a stream id of the stochastic forms); ValueError for anything else, bools included"""
    if not isinstance(value, int) or isinstance(value, bool) or not 0 <= value < 1 << 64:
        raise ValueError(f"{what}: {name} must be a Python int in [0, 2**64), got {value!r}")
    return value


def mx_quantize_sr(x, fmt, seed, stream=0, scale_rule="floor", axis=-1):
    """mx_quantize_axis with STOCHASTIC rounding onto the element grid: every element becomes one of its two grid
    neighbours, the upper one with probability (distance to the lower) / (their distance) in steps of 2^-16, so E[y] = x where nearest
    rounding sends every element below half a quantum to zero -- the rule for a gradient.  Values on the grid are unchanged.  Under
    scale_rule="ceil" nothing saturates and the whole block is unbiased; under "floor" the top binade of a block still clips.
    The noise is Philox4x32-10 on (seed, stream, flat index of the element in the contiguous tensor): Python ints in [0, 2^64), the same
    pair gives the same bits.  A non-contiguous or misaligned input is copied once (mx_copy_route) and gives the bits of its contiguous
    equal; along axis=-2 the last dimension must be whole 16-byte vectors (ValueError).  One launch (mx_sr_launch / mx_sr_cols_launch);
    no rotation, no mask.  -> a new contiguous tensor of x's shape and dtype."""
    what = "mx_quantize_sr"
    down = isinstance(x, torch.Tensor) and check_mx_axis(x.dim(), axis, what) == -2
    flags = check_mx_scale_rule(scale_rule, what)
    seed, stream = check_mx_sr_word(seed, "seed"), check_mx_sr_word(stream, "stream")
    x, code, dt, _ = _mx_input(x, fmt, what, False, -2 if down else -1, True)
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    entry, counter = ("fqs_mx_fwd_cols", "mx_sr_cols_launch") if down else ("fqs_mx_fwd", "mx_sr_launch")
    _mx_launch(what, entry, counter, x, (x.data_ptr(), y.data_ptr()), code, dt, flags, seed, stream)
    return y


def check_mx_ste(g_shape, mask_shape, mask_dtype, rotate):
    """The argument checks of mx_ste_backward on shapes alone (the fake implementation of the compiled op runs them too)."""
    if len(g_shape) == 0 or g_shape[-1] % MX_BLOCK:
        raise ValueError(f"mx_ste_backward: the gradient needs a last dimension that is a multiple of {MX_BLOCK}, got shape {tuple(g_shape)}")
    if rotate:
        check_mx_rotate(tuple(g_shape), "mx_ste_backward")
    if mask_dtype != torch.uint8:
        raise TypeError(f"mx_ste_backward: the mask is a uint8 bitmap (mx_quantize(return_mask=True)), got {mask_dtype}")
    n = 1
    for d in g_shape:
        n *= d
    m = 1
    for d in mask_shape:
        m *= d
    if m * 8 != n:
        raise ValueError(f"mx_ste_backward: the mask holds {m} bytes, the gradient {n} elements: one bit per element is {n // 8} bytes")


def mx_ste_backward(g, mask, rotate=False):
    """The straight-through gradient of mx_quantize under its saturation mask: g where the element's bit is 1, +0.0 where it is 0 (a
    select: a NaN / Inf g there gives +0.0).  rotate=True: the masked gradient times R, rounded once to g's dtype -- mx_rotate of the
    masked gradient bit for bit, in the same single launch.  -> a new tensor of g's shape and dtype."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"mx_ste_backward: expected a torch.Tensor mask, got {type(mask).__name__}")
    if isinstance(g, torch.Tensor):
        check_mx_ste(tuple(g.shape), tuple(mask.shape), mask.dtype, rotate)
    g, _, dt, _ = _mx_input(g, None, "mx_ste_backward")
    if mask.device != g.device:
        raise RuntimeError(f"mx_ste_backward: the mask is on '{mask.device}', the gradient on '{g.device}'")
    mask = _mx_aligned(mask, True)
    gx = torch.empty_like(g, memory_format=torch.contiguous_format)
    flags = _lib.MX_FLAG_ROTATE if rotate else 0
    _mx_launch("mx_ste_backward", "fq_mx_ste_bwd", "mx_ste_launch", g, (g.data_ptr(), mask.data_ptr(), gx.data_ptr()), dt, flags)
    return gx


# E2M1 values of the 16 FP4 codes (sign in bit 3)
_FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


class MXExport:
    """The integer form of an MX-fake-quantized tensor.
      elements  uint8 [..., cols / 2] (mxfp4: element 2k in the low nibble of byte k) or [..., cols] (mxfp8_*: float8_e4m3fn / float8_e5m2
                bit patterns)
      scales    uint8 [..., cols / 32]: one E8M0 byte (E + 127) per block; 0xFF marks a block that held a NaN or Inf (its codes are 0)
      rotated   the export is of x R (mx_export(..., rotate=True)): its values live in the rotated basis
    dequantize() gives back mx_quantize(x, fmt, rotate=rotated) bit for bit (signed zeros included; NaN blocks as NaN), in plain torch ops."""
    __slots__ = ("elements", "scales", "fmt", "shape", "dtype", "rotated")

    def __init__(self, elements, scales, fmt, shape, dtype, rotated=False):
        self.elements, self.scales, self.fmt, self.shape, self.dtype = elements, scales, fmt, tuple(shape), dtype
        self.rotated = bool(rotated)

    def __repr__(self):
        return f"MXExport(fmt={self.fmt!r}, shape={self.shape}, dtype={self.dtype}{', rotated=True' if self.rotated else ''})"

    def dequantize(self):
        e = self.elements
        if self.fmt == "mxfp4":
            lut = torch.tensor(_FP4_VALUES, dtype=torch.float32, device=e.device)
            codes = torch.stack((e & 0xF, e >> 4), -1).reshape(*e.shape[:-1], e.shape[-1] * 2)
            q = lut[codes.long()]
        elif self.fmt in ("mxfp8_e4m3", "mxfp8_e5m2"):
            q = e.view(torch.float8_e4m3fn if self.fmt == "mxfp8_e4m3" else torch.float8_e5m2).float()
        else:
            raise ValueError(f"{self.fmt!r} has no export packing")
        # 2^(scale - 127), built from its float32 bits (exact: 0 -> 2^-127, a subnormal); the E8M0 NaN byte 0xFF -> NaN for the whole block
        s = self.scales.int()
        x = torch.where(s == 0, 0x00400000, s << 23).view(torch.float32)
        x = torch.where(s == 0xFF, float("nan"), x)
        y = q.view(*q.shape[:-1], -1, MX_BLOCK) * x.unsqueeze(-1)
        return y.reshape(self.shape).to(self.dtype)


def mx_export(x, fmt, rotate=False, scale_rule="floor"):
    """-> MXExport(elements, scales, fmt, shape, dtype, rotated): the codes and E8M0 scales of mx_quantize(x, fmt, rotate, scale_rule).
    mxfp4 and mxfp8_* only (FP6 has no packing here: ValueError).  The export does not record the rule: dequantize() and mx_matmul read
    whatever scale byte it wrote."""
    flags = check_mx_scale_rule(scale_rule, "mx_export") | (_lib.MX_FLAG_ROTATE if rotate else 0)
    code = check_mx(tuple(x.shape), fmt) if isinstance(x, torch.Tensor) else None
    if code in (_lib.MX_FP6_E2M3, _lib.MX_FP6_E3M2):
        raise ValueError(f"{fmt!r}: FP6 formats have no export packing")
    x, _, dt, _ = _mx_input(x, None, "mx_export", rotate)   # (the format is checked: the FP6 refusal comes before the rotation's and the device's)
    cols = x.shape[-1]
    lead = tuple(x.shape[:-1])
    elems = torch.empty(lead + (cols // 2 if code == _lib.MX_FP4_E2M1 else cols,), dtype=torch.uint8, device=x.device)
    scales = torch.empty(lead + (cols // MX_BLOCK,), dtype=torch.uint8, device=x.device)
    _mx_launch("mx_export", "fq_mx_export_ex", "mx_export_launch", x, (x.data_ptr(), elems.data_ptr(), scales.data_ptr()), code, dt, flags)
    return MXExport(elems, scales, fmt, tuple(x.shape), x.dtype, rotate)


# ---- an export back to a tensor in one launch (fqi_mx_dequant of the fourth header) --------------------------------
def check_mx_dequant(fmt, shape, dtype):
    """The argument checks of mx_dequantize on shapes alone (the fake implementation of the compiled op runs them too) -> the number of
    elements: ValueError for an unknown or an FP6 format, a dtype that is not served, a last dimension that is not whole blocks."""
    if fmt not in MX_FORMATS:
        raise ValueError(f"mx_dequantize: unknown MX format {fmt!r}: one of {', '.join(MX_GEMM_FORMATS)}")
    if fmt not in MX_GEMM_FORMATS:
        raise ValueError(f"mx_dequantize: {fmt!r}: FP6 formats have no export packing")
    if dtype not in _OUT_DTYPES:
        raise ValueError(f"mx_dequantize: dtype {dtype} is not served (float32, bfloat16, float16 are)")
    if len(shape) == 0 or shape[-1] % MX_BLOCK:
        raise ValueError(f"mx_dequantize: the shape needs a last dimension that is a multiple of {MX_BLOCK}, got {tuple(shape)}")
    n = 1
    for d in shape:
        n *= d
    return n


def mx_dequantize_tensors(elements, scales, fmt, shape, dtype):
    """mx_dequantize on the export's tensors (what MXLinear keeps as buffers): `elements` and `scales` are the uint8 code and E8M0 bytes
    of a contiguous tensor of `shape` in `fmt`, in any shape of their own that holds those bytes in order.  -> a new contiguous tensor of
    `shape` and `dtype`.  One launch (mx_dequant_launch); a non-contiguous or misaligned buffer is copied once first (mx_copy_route); an
    empty shape launches nothing."""
    shape = tuple(shape)
    n = check_mx_dequant(fmt, shape, dtype)
    for t in (elements, scales):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError("mx_dequantize: elements and scales are uint8 tensors")
    if elements.numel() != (n // 2 if fmt == "mxfp4" else n):
        raise ValueError(f"mx_dequantize: elements holds {elements.numel()} bytes, not those of a {list(shape)} {fmt} export")
    if scales.numel() != n // MX_BLOCK:
        raise ValueError(f"mx_dequantize: scales holds {scales.numel()} bytes, not one per {MX_BLOCK}-element block of a {list(shape)} tensor")
    for t in (elements, scales):
        _prep_u8(t, "mx_dequantize")      # the device: no CPU implementation
    if elements.device != scales.device:
        raise ValueError("mx_dequantize: elements and scales live on different devices")
    elements, scales = _mx_aligned(elements, True), _mx_aligned(scales, True)
    y = torch.empty(shape, dtype=dtype, device=elements.device)
    _mx_launch("mx_dequantize", "fqi_mx_dequant", "mx_dequant_launch", elements, (elements.data_ptr(), scales.data_ptr(), y.data_ptr()),
               MX_FORMATS[fmt], _OUT_DTYPES[dtype], dims=(n // shape[-1] if shape[-1] else 0, shape[-1]))
    return y


def mx_dequantize(e, dtype=None):
    """The tensor an MXExport stands for, in one launch: e.dequantize() bit for bit (any NaN for a NaN), of e.shape and `dtype` (default
    e.dtype) -- so mx_dequantize(mx_export(x, fmt, rotate, rule)) is mx_quantize(x, fmt, rotate, rule), in the rotated basis where the
    export is.  Every element is the value of its code times 2^(scale byte - 127) in fp32 (exact), rounded once to the dtype."""
    if not isinstance(e, MXExport):
        raise TypeError("mx_dequantize: e is an MXExport object (ops.mx_export)")
    return mx_dequantize_tensors(e.elements, e.scales, e.fmt, e.shape, e.dtype if dtype is None else dtype)


# ---- MX block-scaled GEMM: the exported codes on gfx950's scaled matrix instruction (fq_mx_gemm) ------------------
MX_GEMM_KSTEP = 128      # k of one v_mfma_scale_f32_16x16x128_f8f6f4: K must be a multiple
MX_GEMM_SKINNY_M = 32    # rows of `a` up to which the skinny (decode) kernel runs
MX_GEMM_FORMATS = ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2")
_OUT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}   # what the GEMM and the dequantize write, and the logits the losses read


def check_mx_matmul(a_shape, a_fmt, w_shape, w_fmt, out_dtype):
    """The argument checks of mx_matmul on shapes alone (the fake implementation of the compiled op runs them too) -> (M, N, K)."""
    for what, fmt in (("a", a_fmt), ("w", w_fmt)):
        if fmt not in MX_FORMATS:
            raise ValueError(f"mx_matmul: unknown MX format {fmt!r} of {what}: one of {', '.join(MX_GEMM_FORMATS)}")
        if fmt not in MX_GEMM_FORMATS:
            raise ValueError(f"mx_matmul: {fmt!r} ({what}): FP6 formats have no export packing and are no GEMM operand")
    if len(w_shape) != 2:
        raise ValueError(f"mx_matmul: w must be 2-D [N, K], got shape {tuple(w_shape)}")
    if len(a_shape) < 1:
        raise ValueError("mx_matmul: a needs at least one dimension")
    K = a_shape[-1]
    if K != w_shape[1]:
        raise ValueError(f"mx_matmul: a has K={K} but w has K={w_shape[1]}")
    if K == 0 or K % MX_GEMM_KSTEP:
        raise ValueError(f"mx_matmul: K={K} is not served: the kernel needs a positive multiple of {MX_GEMM_KSTEP}")
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"mx_matmul: out_dtype {out_dtype} is not served (float32, bfloat16, float16 are)")
    M = 1
    for d in a_shape[:-1]:
        M *= d
    return M, w_shape[0], K


def mx_matmul_tensors(a_elems, a_scales, a_fmt, w_elems, w_scales, w_fmt, a_shape, out_dtype):
    """mx_matmul on the exports' tensors (what MXLinear keeps as buffers); a_shape: the exported activation's shape [..., K]."""
    w_shape = (w_scales.shape[0], w_scales.shape[1] * MX_BLOCK) if w_scales.dim() == 2 else tuple(w_scales.shape)   # [N, K / 32] bytes
    M, N, K = check_mx_matmul(tuple(a_shape), a_fmt, w_shape, w_fmt, out_dtype)
    ts = (a_elems, a_scales, w_elems, w_scales)
    for t in ts:
        _prep_u8(t, "mx_matmul")
    if len({t.device for t in ts}) != 1:
        raise ValueError("mx_matmul: the operands live on different devices")
    for t, fmt, rows, what in ((a_elems, a_fmt, M, "a.elements"), (w_elems, w_fmt, N, "w.elements")):
        if t.numel() != rows * (K // 2 if fmt == "mxfp4" else K):
            raise ValueError(f"mx_matmul: {what} holds {t.numel()} bytes, not those of a [{rows}, {K}] {fmt} export")
    if a_scales.numel() != M * (K // MX_BLOCK) or w_scales.numel() != N * (K // MX_BLOCK):
        raise ValueError("mx_matmul: a scales tensor does not hold one byte per 32-element block")
    a_elems, a_scales, w_elems, w_scales = (_mx_aligned(t, False) for t in ts)
    out = torch.empty(tuple(a_shape[:-1]) + (N,), dtype=out_dtype, device=a_elems.device)
    head = (a_elems.data_ptr(), a_scales.data_ptr(), MX_FORMATS[a_fmt], w_elems.data_ptr(), w_scales.data_ptr(), MX_FORMATS[w_fmt], out.data_ptr())
    if _mx_launch("mx_matmul", "fq_mx_gemm", "mx_gemm_launch", a_elems, head, _OUT_DTYPES[out_dtype], dims=(M, N, K)):
        mx_counts["mx_gemm_skinny" if M <= MX_GEMM_SKINNY_M else "mx_gemm_tiled"] += 1
    return out


def _prep_u8(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError(f"{what}: elements and scales are uint8 tensors")
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: tensor is on '{t.device}'. llm_qat_amd runs on MI355X only and has no CPU "
                           "fallback; move the tensor to the GPU.")


def mx_matmul(a, w, out_dtype=None):
    """out[..., n] = sum_k a[..., k] * w[n, k] over two MXExports, on the block-scaled matrix instruction: the value of
    a.dequantize().double() @ w.dequantize().double().T up to the fp32 accumulation of the matrix core, rounded once to out_dtype
    (default a.dtype).  a: [..., K], w: [N, K], each mxfp4 / mxfp8_e4m3 / mxfp8_e5m2; K a multiple of 128.  An 0xFF (NaN) scale block in a
    row of a / w makes that output row / column NaN.  Both operands rotated or neither (ValueError): (a R)(w R)^T = a w^T, a R w^T is not.
    The contract covers what mx_export emits: finite element codes and scale bytes 0 .. 254 (byte 0 is 2^-127) or 0xFF.  Measured over
    every code and byte: a single product outside fp32's normal range comes out rounded once (gradual underflow,
    +-Inf above the maximum); the FP8 NaN / Inf codes, which mx_export never writes, act as IEEE NaN / +-Inf (Inf x 0 = NaN)."""
    if not isinstance(a, MXExport) or not isinstance(w, MXExport):
        raise TypeError("mx_matmul: a and w are MXExport objects (ops.mx_export)")
    if a.rotated != w.rotated:
        raise ValueError(f"mx_matmul: a is {'rotated' if a.rotated else 'not rotated'} and w is {'rotated' if w.rotated else 'not rotated'}: "
                         "the product only equals the unrotated one when both operands carry the same rotation")
    out_dtype = a.dtype if out_dtype is None else out_dtype
    check_mx_matmul(a.shape, a.fmt, w.shape, w.fmt, out_dtype)
    return mx_matmul_tensors(a.elements, a.scales, a.fmt, w.elements, w.scales.reshape(w.shape[0], -1), w.fmt, a.shape, out_dtype)


# ---- what the row operations share, the fused losses and the norm (DESIGN.md sections 24 and 26) ------------------------------------------
def _row_tensors(what, **named):
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name}: expected a torch.Tensor, got {type(t).__name__}")


def _row_contig(t, counts):   # the copy route: a non-contiguous tensor is copied once, and counted
    if not t.is_contiguous():
        counts["copy_route"] += 1
    return t.contiguous()


def _row_stats(what, t, name, shape, like):   # the forward's row statistics (name: "<argument> is <forward>'s") as the backward wants them
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape and t.device == like.device and t.is_contiguous()):
        raise ValueError(f"{what}: {name} contiguous fp32 {list(shape)} tensor on {like.device}")


# ---- what only the fused losses share.  The argument checks stand one by one, because each loss puts checks of its own between them and
# the order of its refusals is pinned: one message each, whatever the order -------------------------------------------------------------
def _loss_dtype(what, logits):
    if logits.dtype not in _OUT_DTYPES:
        raise TypeError(f"{what}: dtype {logits.dtype} is not served (float32, bfloat16, float16 are; the arithmetic is fp32 for all three)")


def _loss_dims(what, logits, layout):
    if logits.dim() < 2:
        raise ValueError(f"{what}: the logits need at least two dimensions {layout}, got {tuple(logits.shape)}")


def _loss_not_empty(what, logits):
    if logits.numel() == 0:
        raise ValueError(f"{what}: empty logits {tuple(logits.shape)}: a loss has no empty launch")


def _loss_grad(what, grad_loss, logits):   # the upstream gradient as the kernel reads it on the device: detached, fp32, [1]
    if not (isinstance(grad_loss, torch.Tensor) and grad_loss.numel() == 1 and grad_loss.device == logits.device):
        raise ValueError(f"{what}: grad_loss is a one-element tensor on {logits.device}")
    g = grad_loss.detach().reshape(1)
    return g if g.dtype == torch.float32 else g.float()


# ---- the distillation loss kl_div(log_softmax(student), softmax(teacher), "batchmean") (the fql_ header) ----------
kd_counts = {"fwd_launch": 0, "bwd_launch": 0, "copy_route": 0}


def check_kd(student, teacher, what="kd_kl_loss"):
    """The argument checks of the loss on types, shapes and dtypes alone (the fake implementations of the compiled ops run them too) ->
    (rows, cols, batch): TypeError for a non-tensor, mixed dtypes or a dtype that is not served (float64 among them), ValueError for
    unequal shapes, fewer than two dimensions, an empty shape, or a teacher that requires grad while grad mode is on."""
    _row_tensors(what, student_logits=student, teacher_logits=teacher)
    if student.dtype != teacher.dtype:
        raise TypeError(f"{what}: mixed dtypes are not served: student_logits is {student.dtype}, teacher_logits is {teacher.dtype}")
    _loss_dtype(what, student)
    if tuple(student.shape) != tuple(teacher.shape):
        raise ValueError(f"{what}: shape mismatch: student_logits {tuple(student.shape)}, teacher_logits {tuple(teacher.shape)}")
    _loss_dims(what, student, "[batch, ..., vocabulary]")
    _loss_not_empty(what, student)
    if teacher.requires_grad and torch.is_grad_enabled():
        raise ValueError(f"{what}: teacher_logits requires grad: the loss has no gradient for the teacher; pass teacher_logits.detach()")
    cols = student.shape[-1]
    return student.numel() // cols, cols, student.shape[0]


def kd_inputs(student, teacher, what="kd_kl_loss"):
    """check_kd, then the device (CUDA, the same one), then the copy route: a non-contiguous tensor is copied once (copy_route)
    -> (student, teacher, rows, cols, batch)"""
    rows, cols, batch = check_kd(student, teacher, what)
    _prep(student, what)
    _prep(teacher, what)
    if student.device != teacher.device:
        raise ValueError(f"{what}: student_logits is on {student.device}, teacher_logits on {teacher.device}")
    return _row_contig(student, kd_counts), _row_contig(teacher, kd_counts), rows, cols, batch


def kd_kl_forward(student, teacher, need_stats=True):
    """-> (loss, row_stats, row_loss): the fp32 0-dim loss, the [rows, 2] fp32 (lse_s, lse_t) the backward reads (None with
    need_stats=False: no buffer, nothing written) and the [rows] fp32 row losses, rows = numel / shape[-1].  fp32 arithmetic whatever
    the logits' dtype; two launches on the current stream (the rows, the sum), counted as one fwd_launch."""
    student, teacher, rows, cols, batch = kd_inputs(student, teacher, "kd_kl_forward")
    side = torch.empty(rows * (3 if need_stats else 1) + 1, dtype=torch.float32, device=student.device)   # row_stats | row_loss | loss
    stats = side[:2 * rows].view(rows, 2) if need_stats else None
    row_loss, loss = side[-rows - 1:-1], side[-1]
    rc = _launch(student, _lib.lib().fql_kd_kl_fwd, student.data_ptr(), teacher.data_ptr(), stats.data_ptr() if need_stats else None,
                 row_loss.data_ptr(), loss.data_ptr(), rows, cols, batch, _OUT_DTYPES[student.dtype])
    _lib.check(rc, "kd_kl_forward")
    kd_counts["fwd_launch"] += 1
    return loss, stats, row_loss


def kd_kl_backward(student, teacher, row_stats, grad_loss):
    """-> grad_student = (grad_loss / batch) (softmax(student) - softmax(teacher)), of student's shape and dtype, rounded once from fp32.
    row_stats: kd_kl_forward's, on the same logits; grad_loss: the upstream gradient of the loss, a one-element CUDA tensor that the kernel
    reads on the device (no host synchronisation).  One launch (bwd_launch)."""
    with torch.no_grad():
        student, teacher, rows, cols, batch = kd_inputs(student, teacher, "kd_kl_backward")
    _row_stats("kd_kl_backward", row_stats, "row_stats is kd_kl_forward's", (rows, 2), student)
    g = _loss_grad("kd_kl_backward", grad_loss, student)
    grad = torch.empty_like(student)
    rc = _launch(student, _lib.lib().fql_kd_kl_bwd, student.data_ptr(), teacher.data_ptr(), row_stats.data_ptr(), g.data_ptr(), grad.data_ptr(),
                 rows, cols, batch, _OUT_DTYPES[student.dtype])
    _lib.check(rc, "kd_kl_backward")
    kd_counts["bwd_launch"] += 1
    return grad


# ---- the language-model loss cross_entropy(logits, labels, ignore_index), the causal shift in the kernel (the fqc_ header) ----
ce_counts = {"fwd_launch": 0, "bwd_launch": 0, "copy_route": 0}
_CE_REDUCTIONS = {"mean": _lib.CE_MEAN, "sum": _lib.CE_SUM}
_CE_SERVED = ("int64 class-index labels with ignore_index and reduction 'mean' or 'sum' are served; class weights, label smoothing, "
              "probability targets and reduction='none' are not")


def check_ce(logits, labels, shift=False, ignore_index=-100, reduction="mean", what="cross_entropy"):
    """The argument checks of the loss on types, shapes and dtypes alone (the fake implementations of the compiled ops run them too) ->
    (rows, cols, seq_len): TypeError for a non-tensor, a logits dtype that is not served (float64 among them), labels that are not int64
    (probability targets among them) or an ignore_index that is no int; ValueError for fewer than two dimensions, labels that are not of
    the logits' shape without its last dimension, an empty shape, or a reduction other than 'mean' and 'sum'."""
    _row_tensors(what, logits=logits, labels=labels)
    _loss_dtype(what, logits)
    if labels.dtype != torch.int64:
        raise TypeError(f"{what}: labels of dtype {labels.dtype} are not served: {_CE_SERVED}")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise TypeError(f"{what}: ignore_index is an int, got {type(ignore_index).__name__}")
    if reduction not in _CE_REDUCTIONS:
        raise ValueError(f"{what}: reduction={reduction!r} is not served: {_CE_SERVED}")
    _loss_dims(what, logits, "[..., positions, vocabulary]")
    if tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"{what}: shape mismatch: logits {tuple(logits.shape)} want labels {tuple(logits.shape[:-1])}, got {tuple(labels.shape)}")
    _loss_not_empty(what, logits)
    cols = logits.shape[-1]
    return logits.numel() // cols, cols, logits.shape[-2]


def ce_inputs(logits, labels, shift=False, ignore_index=-100, reduction="mean", what="cross_entropy"):
    """check_ce, then the device (CUDA, the same one), then the copy route: a non-contiguous tensor is copied once (copy_route)
    -> (logits, labels, rows, cols, seq_len)"""
    rows, cols, seq_len = check_ce(logits, labels, shift, ignore_index, reduction, what)
    _prep(logits, what)
    if labels.device != logits.device:
        raise ValueError(f"{what}: logits are on {logits.device}, labels on {labels.device}")
    return _row_contig(logits, ce_counts), _row_contig(labels, ce_counts), rows, cols, seq_len


def ce_forward(logits, labels, shift=False, ignore_index=-100, reduction="mean", need_stats=True):
    """-> (loss, row_lse, row_loss, n_valid): the fp32 0-dim loss, the [rows] fp32 logsumexp of every valid row that the backward reads
    (None with need_stats=False: no buffer, nothing written), the [rows] fp32 row losses (0 for ignored rows) and the int64 [1] count
    of valid rows, rows = numel / shape[-1]; all four are views of one buffer.  shift: row r is scored against labels[r + 1] and the
    last position of every sequence (shape[-2] positions) is ignored.  fp32 arithmetic whatever the logits' dtype; two launches on the
    current stream (the rows, the sum and the count), counted as one fwd_launch."""
    logits, labels, rows, cols, seq_len = ce_inputs(logits, labels, shift, ignore_index, reduction, "ce_forward")
    side = torch.empty(2 + rows * (2 if need_stats else 1) + 1, dtype=torch.float32, device=logits.device)   # n_valid | row_lse | row_loss | loss
    n_valid = side[:2].view(torch.int64)
    row_lse = side[2:2 + rows] if need_stats else None
    row_loss, loss = side[-rows - 1:-1], side[-1]
    rc = _launch(logits, _lib.lib().fqc_ce_fwd, logits.data_ptr(), labels.data_ptr(), row_lse.data_ptr() if need_stats else None,
                 row_loss.data_ptr(), loss.data_ptr(), n_valid.data_ptr(), rows, cols, seq_len, int(bool(shift)), ignore_index,
                 _CE_REDUCTIONS[reduction], _OUT_DTYPES[logits.dtype])
    _lib.check(rc, "ce_forward")
    ce_counts["fwd_launch"] += 1
    return loss, row_lse, row_loss, n_valid


def ce_backward(logits, labels, row_lse, n_valid, grad_loss, shift=False, ignore_index=-100, reduction="mean"):
    """-> grad_logits = (grad_loss / n) (softmax(logits) - onehot(label)) for valid rows (the divisor is 1 under 'sum'), zeros for ignored
    ones, of the logits' shape and dtype, rounded once from fp32.  row_lse, n_valid: ce_forward's, on the same logits, labels and
    settings; grad_loss: the upstream gradient of the loss, a one-element CUDA tensor that the kernel reads on the device, as it reads
    n_valid (no host synchronisation).  One launch (bwd_launch)."""
    with torch.no_grad():
        logits, labels, rows, cols, seq_len = ce_inputs(logits, labels, shift, ignore_index, reduction, "ce_backward")
    _row_stats("ce_backward", row_lse, "row_lse is ce_forward's", (rows,), logits)
    if not (isinstance(n_valid, torch.Tensor) and n_valid.dtype == torch.int64 and n_valid.numel() == 1 and n_valid.device == logits.device):
        raise ValueError(f"ce_backward: n_valid is ce_forward's one-element int64 tensor on {logits.device}")
    g = _loss_grad("ce_backward", grad_loss, logits)
    grad = torch.empty_like(logits)
    rc = _launch(logits, _lib.lib().fqc_ce_bwd, logits.data_ptr(), labels.data_ptr(), row_lse.data_ptr(), n_valid.data_ptr(), g.data_ptr(),
                 grad.data_ptr(), rows, cols, seq_len, int(bool(shift)), ignore_index, _CE_REDUCTIONS[reduction], _OUT_DTYPES[logits.dtype])
    _lib.check(rc, "ce_backward")
    ce_counts["bwd_launch"] += 1
    return grad


# ---- the RMSNorm  w * (x * rsqrt(mean(x^2) + eps))  in front of the quantized projections (the fqn_ header) ----------
norm_counts = {"fwd_launch": 0, "bwd_launch": 0, "copy_route": 0}
_NORM_SERVED = "equal dtypes (float32, bfloat16, float16) and the pairs in which exactly one of x and weight is float32 are served"


def check_rms_norm(x, w, eps=1e-6, what="rms_norm"):
    """The argument checks of the norm on types, shapes and dtypes alone (the fake implementations of the compiled ops run them too) ->
    (rows, cols): TypeError for a non-tensor, a dtype or a dtype pair that is not served (float64 and bfloat16 with float16 among them) or
    an eps that is no number; ValueError for an eps that is negative, NaN or inf, a weight that is not 1-D, an x whose last dimension is
    not the weight's length, or an empty shape."""
    _row_tensors(what, x=x, weight=w)
    for name, t in (("x", x), ("weight", w)):
        if t.dtype not in _OUT_DTYPES:
            raise TypeError(f"{what}: {name} of dtype {t.dtype} is not served: {_NORM_SERVED}; the arithmetic is fp32 for all of them")
    if x.dtype != w.dtype and torch.float32 not in (x.dtype, w.dtype):
        raise TypeError(f"{what}: the dtype pair (x {x.dtype}, weight {w.dtype}) is not served: {_NORM_SERVED}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)):
        raise TypeError(f"{what}: eps is a number, got {type(eps).__name__}")
    if not 0 <= eps < float("inf"):
        raise ValueError(f"{what}: eps={eps} must be finite and not negative")
    if w.dim() != 1:
        raise ValueError(f"{what}: weight is 1-D [hidden], got shape {tuple(w.shape)}")
    if x.dim() < 1 or x.shape[-1] != w.shape[0]:
        raise ValueError(f"{what}: shape mismatch: x {tuple(x.shape)} wants a weight of {x.shape[-1] if x.dim() else '?'} elements, got {w.shape[0]}")
    if x.numel() == 0:
        raise ValueError(f"{what}: empty x {tuple(x.shape)}: a norm has no empty launch")
    return x.numel() // w.shape[0], w.shape[0]


def rms_norm_inputs(x, w, eps=1e-6, what="rms_norm"):
    """check_rms_norm, then the device (CUDA, the same one), then the copy route: a non-contiguous tensor is copied once (copy_route)
    -> (x, w, rows, cols)"""
    rows, cols = check_rms_norm(x, w, eps, what)
    _prep(x, what)
    _prep(w, what)
    if x.device != w.device:
        raise ValueError(f"{what}: x is on {x.device}, weight on {w.device}")
    return _row_contig(x, norm_counts), _row_contig(w, norm_counts), rows, cols


def rms_norm_forward(x, w, eps=1e-6, need_stats=True):
    """-> (y, rstd): y = w * (x * rsqrt(mean(x^2, -1) + eps)) of x's shape and w's dtype, in fp32 arithmetic with the reference chain's
    roundings, and the fp32 [rows] rstd the backward reads (None with need_stats=False: no buffer, nothing written),
    rows = numel / shape[-1].  One launch on the current stream (fwd_launch)."""
    x, w, rows, cols = rms_norm_inputs(x, w, eps, "rms_norm_forward")
    y = torch.empty(x.shape, dtype=w.dtype, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if need_stats else None
    rc = _launch(x, _lib.lib().fqn_rms_norm_fwd, x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr() if need_stats else None, rows, cols,
                 float(eps), _OUT_DTYPES[x.dtype], _OUT_DTYPES[w.dtype])
    _lib.check(rc, "rms_norm_forward")
    norm_counts["fwd_launch"] += 1
    return y, rstd


def rms_norm_backward(g, x, w, rstd, need_dx=True, need_dw=True):
    """-> (dx, dw): with a = g w, n = x rstd and s = mean(a n, -1): dx = rstd (a - n s) of x's shape and dtype, dw = sum over the rows of
    g n of w's shape and dtype, each rounded once from fp32; None for the one that is not needed (need_dw=False: no partial sums, no second
    launch, no workspace).  g: the gradient of rms_norm_forward's y (its shape, w's dtype); rstd: rms_norm_forward's, on the same x and
    eps.  No atomics: two calls give the same bits.  The workspace comes from the caching allocator.  Counted as one bwd_launch."""
    with torch.no_grad():
        x, w, rows, cols = rms_norm_inputs(x, w, 0.0, "rms_norm_backward")
    if not (need_dx or need_dw):
        raise ValueError("rms_norm_backward: neither dx nor dw is asked for")
    _row_tensors("rms_norm_backward", g=g)
    if g.dtype != w.dtype or tuple(g.shape) != tuple(x.shape) or g.device != x.device:
        raise ValueError(f"rms_norm_backward: g is the gradient of y: {tuple(x.shape)} of {w.dtype} on {x.device}, got {tuple(g.shape)} of {g.dtype} on {g.device}")
    _row_stats("rms_norm_backward", rstd, "rstd is rms_norm_forward's", (rows,), x)
    g = _row_contig(g.detach(), norm_counts)
    L = _lib.lib()
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dw else None
    ws_bytes = L.fqn_rms_norm_bwd_workspace_bytes(rows, cols) if need_dw else 0
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device) if need_dw else None
    rc = _launch(x, L.fqn_rms_norm_bwd, g.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr() if need_dx else None,
                 dw.data_ptr() if need_dw else None, ws.data_ptr() if need_dw else None, ws_bytes, rows, cols, _OUT_DTYPES[x.dtype],
                 _OUT_DTYPES[w.dtype])
    _lib.check(rc, "rms_norm_backward")
    norm_counts["bwd_launch"] += 1
    return dx, dw


# ---- the gated activation  silu(gate) * up  of the MLP (the fqa_ header) --------------------------------------------------
class _ActCounts:
    """fwd_launch / bwd_launch / copy_route as a mapping: what this module counted plus what the C++ node of mlp.swiglu counted (its
    backward runs on the autograd engine's thread without the GIL and cannot touch a dict)"""
    _KEYS = ("fwd_launch", "bwd_launch", "copy_route")

    def __init__(self):
        self._own = dict.fromkeys(self._KEYS, 0)

    def __getitem__(self, key):
        from . import _act_node
        return self._own[key] + _act_node.counters()[self._KEYS.index(key)]

    def __setitem__(self, key, value):       # counts[key] += 1: the node's share stays the node's
        from . import _act_node
        self._own[key] = value - _act_node.counters()[self._KEYS.index(key)]

    def keys(self):
        return self._KEYS

    def __iter__(self):
        return iter(self._KEYS)

    def __len__(self):
        return len(self._KEYS)

    def __eq__(self, other):
        return dict(self) == dict(other)

    def __repr__(self):
        return repr(dict(self))


act_counts = _ActCounts()


def check_swiglu(gate, up, what="swiglu"):
    """The argument checks of the activation on types, shapes and dtypes alone (the fake implementations of the compiled ops run them
    too) -> (rows, cols), (0, 0) for an empty shape: TypeError for a non-tensor, a dtype that is not served (float64 and the integer
    dtypes among them) or unequal dtypes (no promotion); ValueError for unequal shapes (no broadcasting), a 0-dim tensor, or tensors on
    different devices."""
    if (type(gate) is torch.Tensor and type(up) is torch.Tensor and gate.dtype is up.dtype and gate.dtype in _OUT_DTYPES and gate.shape == up.shape
            and gate.dim() >= 1 and gate.device == up.device and gate.numel()):       # the call that is served, in one line; else: which refusal
        return gate.numel() // gate.shape[-1], gate.shape[-1]
    _row_tensors(what, gate=gate, up=up)
    for name, t in (("gate", gate), ("up", up)):
        if t.dtype not in _OUT_DTYPES:
            raise TypeError(f"{what}: {name} of dtype {t.dtype} is not served (float32, bfloat16, float16 are; the arithmetic is fp32 for all three)")
    if gate.dtype != up.dtype:
        raise TypeError(f"{what}: mixed dtypes are not served (no promotion): gate is {gate.dtype}, up is {up.dtype}")
    if tuple(gate.shape) != tuple(up.shape):
        raise ValueError(f"{what}: shape mismatch (no broadcasting): gate {tuple(gate.shape)}, up {tuple(up.shape)}")
    if gate.dim() < 1:
        raise ValueError(f"{what}: the tensors need at least one dimension, got a 0-dim tensor")
    if gate.device != up.device:
        raise ValueError(f"{what}: gate is on {gate.device}, up on {up.device}")
    if gate.numel() == 0:
        return 0, 0
    return gate.numel() // gate.shape[-1], gate.shape[-1]


def _act_rows(t):
    """-> (t or its one copy, row stride in elements): a tensor is served where it lies when its last stride is 1 and its leading
    dimensions collapse to one row stride of at least a row (rows_view); anything else is copied once and counted (copy_route)"""
    cols = t.shape[-1]
    v = rows_view(t)
    if v is None:
        return t, cols
    if v and (t.dim() == 2 or v[1] == v[0] * v[2]) and v[2] >= cols:
        return t, v[2]
    act_counts["copy_route"] += 1
    return t.contiguous(), cols


def swiglu_launch_forward(gate, up, rows, cols):
    """swiglu_forward behind check_swiglu's (rows, cols), for a caller that has run the checks (mlp.swiglu: every microsecond of host time
    before the launch is added to the kernel's, which is shorter than the eager chain's two by some twenty of them) -> (y, gate, up), the
    inputs as the launch read them: each the tensor itself where it is served where it lies, else its one contiguous copy"""
    _prep(gate, "swiglu_forward")
    y = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device)
    if rows == 0:
        return y, gate, up
    (g, sg), (u, su) = _act_rows(gate), _act_rows(up)
    rc = _launch(g, _lib.lib().fqa_swiglu_fwd, g.data_ptr(), u.data_ptr(), y.data_ptr(), rows, cols, sg, su, _OUT_DTYPES[g.dtype])
    _lib.check(rc, "swiglu_forward")
    act_counts["fwd_launch"] += 1
    return y, g, u


def swiglu_forward(gate, up):
    """-> y = silu(gate) * up, contiguous, of gate's shape and dtype: fp32 arithmetic with the roundings of the eager chain
    F.silu(gate) * up, whose bits it gives.  Row views (the halves of gate_up.chunk(2, -1)) are read where they lie.  One launch on the
    current stream (fwd_launch); an empty tensor gives an empty result without one."""
    return swiglu_launch_forward(gate, up, *check_swiglu(gate, up, "swiglu_forward"))[0]


def swiglu_backward(dy, gate, up, need_dgate=True, need_dup=True, checked=None):
    """-> (dgate, dup), contiguous, of gate's shape and dtype, the bits of the eager chain's autograd; None for the one that is not needed
    (neither computed nor stored).  dy: the gradient of swiglu_forward's y (its shape, dtype and device).  One launch (bwd_launch); an
    empty tensor gives empty results without one.  checked: check_swiglu's (rows, cols) of a caller that has run it on gate and up."""
    rows, cols = checked or check_swiglu(gate, up, "swiglu_backward")
    if not (need_dgate or need_dup):
        raise ValueError("swiglu_backward: neither dgate nor dup is asked for")
    _row_tensors("swiglu_backward", dy=dy)
    if dy.dtype != gate.dtype or dy.shape != gate.shape or dy.device != gate.device:
        raise ValueError(f"swiglu_backward: dy is the gradient of y: {tuple(gate.shape)} of {gate.dtype} on {gate.device}, got {tuple(dy.shape)} of {dy.dtype} on {dy.device}")
    _prep(gate, "swiglu_backward")
    dgate = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device) if need_dgate else None
    dup = torch.empty(gate.shape, dtype=gate.dtype, device=gate.device) if need_dup else None
    if rows == 0:
        return dgate, dup
    (d, sd), (g, sg), (u, su) = _act_rows(dy), _act_rows(gate), _act_rows(up)
    rc = _launch(g, _lib.lib().fqa_swiglu_bwd, d.data_ptr(), g.data_ptr(), u.data_ptr(), dgate.data_ptr() if need_dgate else None,
                 dup.data_ptr() if need_dup else None, rows, cols, sd, sg, su, _OUT_DTYPES[g.dtype])
    _lib.check(rc, "swiglu_backward")
    act_counts["bwd_launch"] += 1
    return dgate, dup


# ---- the rotary position embedding of q and k (the fqr_ header) ---------------------------------------------------------
class _RopeCounts(_ActCounts):
    """fwd_launch / bwd_launch / copy_route of the rotary embedding: this module's counts plus those of the C++ node of rope.rotary"""

    def __getitem__(self, key):
        from . import _rope_node
        return self._own[key] + _rope_node.counters()[self._KEYS.index(key)]

    def __setitem__(self, key, value):
        from . import _rope_node
        self._own[key] = value - _rope_node.counters()[self._KEYS.index(key)]


rope_counts = _RopeCounts()


def check_rope_tables(cos, sin, position_ids, lead, B, T, D, what, dtype):
    """check_rope's checks of the tables and positions against a tensor `lead` on the tensors' device; dtype: rope_result_dtype"""
    named = dict(cos=cos, sin=sin)
    if position_ids is not None:
        named["position_ids"] = position_ids
    _row_tensors(what, **named)
    if cos.dtype != sin.dtype or (cos.dtype != dtype and cos.dtype != torch.float32):
        raise TypeError(f"{what}: the tables are both in the tensors' dtype ({dtype}) or both in float32, got {cos.dtype} and {sin.dtype}")
    if tuple(cos.shape) != tuple(sin.shape) or not ((cos.dim() == 2 or (cos.dim() == 4 and cos.shape[0] == cos.shape[1] == 1)) and cos.shape[-1] == D and cos.shape[-2] > 0):
        raise ValueError(f"{what}: the tables are [P, {D}] or [1, 1, P, {D}] with P > 0 and equal shapes, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    if position_ids is not None:
        if position_ids.dtype != torch.int64:
            raise TypeError(f"{what}: position_ids of dtype {position_ids.dtype}: int64 is served")
        if position_ids.dim() != 2 or position_ids.shape[1] != T or position_ids.shape[0] not in (1, B):
            raise ValueError(f"{what}: position_ids are [{B}, {T}] or [1, {T}], got {tuple(position_ids.shape)}")
    for name, t in named.items():
        if t.device != lead.device:
            raise ValueError(f"{what}: the tensors are on {lead.device}, {name} on {t.device}")


def check_rope(q, k, cos, sin, position_ids=None, what="rotary"):
    """The argument checks of the rotary embedding on types, shapes, dtypes and devices alone (the fake implementations of the compiled
    ops run them too) -> (B, Hq, Hk, T, D, P): TypeError for a non-tensor, a dtype that is not served, unequal dtypes of q and k, tables
    that are neither in that dtype nor float32, positions that are not int64; ValueError for shapes (q, k not 4-D or unequal in batch,
    tokens or head size, an odd head size, an empty tensor, tables that are not [P, D] or [1, 1, P, D], positions that are not [B, T] or
    [1, T]) and for tensors on different devices."""
    try:                                                   # the call that is served, in one expression; else: which refusal
        T, D, dev, p = q.shape[2], q.shape[3], q.device, position_ids
        if (type(q) is type(k) is type(cos) is type(sin) is torch.Tensor and q.dtype in _OUT_DTYPES and k.dtype in _OUT_DTYPES
                and (q.dtype is k.dtype or torch.float32 in (q.dtype, k.dtype)) and q.dim() == 4 and k.dim() == 4
                and k.shape[0] == q.shape[0] and k.shape[2] == T and k.shape[3] == D and D % 2 == 0 and q.numel() and k.numel()
                and cos.dtype is sin.dtype and (cos.dtype is torch.float32 or cos.dtype is q.dtype is k.dtype) and cos.shape == sin.shape and cos.shape[-1] == D
                and (cos.dim() == 2 or (cos.dim() == 4 and cos.shape[0] == cos.shape[1] == 1)) and cos.shape[-2] > 0
                and k.device == dev and cos.device == dev and sin.device == dev
                and (p is None or (type(p) is torch.Tensor and p.dtype is torch.int64 and p.dim() == 2 and p.shape[1] == T and p.shape[0] in (1, q.shape[0]) and p.device == dev))):
            return q.shape[0], q.shape[1], k.shape[1], T, D, cos.shape[-2]
    except (AttributeError, IndexError):
        pass
    named = dict(q=q, k=k, cos=cos, sin=sin)
    if position_ids is not None:
        named["position_ids"] = position_ids
    _row_tensors(what, **named)
    for name, t in (("q", q), ("k", k)):
        if t.dtype not in _OUT_DTYPES:
            raise TypeError(f"{what}: {name} of dtype {t.dtype} is not served (float32, bfloat16, float16 are; the arithmetic is fp32 for all three)")
    if q.dtype != k.dtype and torch.float32 not in (q.dtype, k.dtype):
        raise TypeError(f"{what}: q is {q.dtype}, k is {k.dtype}: two dtypes are served where one of them is float32 (the chain then promotes)")
    if q.dim() != 4 or k.dim() != 4:
        raise ValueError(f"{what}: q and k are [B, H, T, D], got {tuple(q.shape)} and {tuple(k.shape)}")
    B, Hq, T, D = q.shape
    if (k.shape[0], k.shape[2], k.shape[3]) != (B, T, D):
        raise ValueError(f"{what}: q and k differ in batch, tokens or head size: {tuple(q.shape)} and {tuple(k.shape)}")
    Hk = k.shape[1]
    if q.numel() == 0 or k.numel() == 0:
        raise ValueError(f"{what}: empty tensors are not served: q {tuple(q.shape)}, k {tuple(k.shape)}")
    if D % 2:
        raise ValueError(f"{what}: odd head size D={D}: a rotation pairs the two halves of a head")
    check_rope_tables(cos, sin, position_ids, q, B, T, D, what, rope_result_dtype(q.dtype, k.dtype))
    if k.device != q.device:
        raise ValueError(f"{what}: q is on {q.device}, k on {k.device}")
    return B, Hq, Hk, T, D, cos.shape[-2]


def rope_result_dtype(q_dtype, k_dtype):
    """the dtype of both results, of both incoming gradients, and the one the tables are rounded to: the tensors' dtype, or float32 where
    q and k differ (one of them then is float32, and the chain promotes)"""
    return q_dtype if q_dtype == k_dtype else torch.float32


def _rope_served(t):
    """-> t, or its one counted copy where the last stride is not 1"""
    if t.stride(-1) == 1 or t.shape[-1] == 1:
        return t
    rope_counts["copy_route"] += 1
    return t.contiguous()


def _rope_table(t, D):
    """-> the table as [P, D] with contiguous rows: a view where it is, else its one counted copy"""
    t = t.reshape(t.shape[-2], D) if t.dim() == 4 else t
    if t.stride(1) == 1 and (t.stride(0) == D or t.shape[0] == 1):
        return t
    rope_counts["copy_route"] += 1
    return t.contiguous()


def _rope_positions(position_ids, B):
    """-> (positions or None, their batch stride in elements)"""
    if position_ids is None:
        return None, 0
    if not position_ids.is_contiguous():
        rope_counts["copy_route"] += 1
        position_ids = position_ids.contiguous()
    return position_ids, (position_ids.shape[1] if position_ids.shape[0] == B and B > 1 else 0)


def rope_dense_like(shape, strides):
    """-> the strides of the dense tensor in the dimension order of a [B, H, T, D] tensor with the given strides: the layout of the
    rotary embedding's results, which is the eager chain's (the rule of include/llmqat_fakequant_rope.h, asked of the library)"""
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.lib().fqr_rope_dense_strides(shape[0], shape[1], shape[2], shape[3], strides[0], strides[1], strides[2], out), "rope_dense_like")
    return (out[0], out[1], out[2], 1)


def rope_launch_forward(q, k, cos, sin, position_ids, geom):
    """rope_forward behind check_rope's geometry, for a caller that has run the checks -> (q_out, k_out, cos, sin, positions, q, k): the
    tables, positions and tensors as the launch read them (a backward needs the first three and the shapes, strides and dtypes of q, k)"""
    B, Hq, Hk, T, D, P = geom
    _prep(q, "rope_forward")
    q, k = _rope_served(q), _rope_served(k)
    cos, sin = _rope_table(cos, D), _rope_table(sin, D)
    pos, pbs = _rope_positions(position_ids, B)
    rdt = rope_result_dtype(q.dtype, k.dtype)
    qo = torch.empty_strided(q.shape, rope_dense_like(q.shape, q.stride()), dtype=rdt, device=q.device)
    ko = torch.empty_strided(k.shape, rope_dense_like(k.shape, k.stride()), dtype=rdt, device=k.device)
    rc = _launch(q, _lib.lib().fqr_rope_fwd, q.data_ptr(), k.data_ptr(), qo.data_ptr(), ko.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                 pos.data_ptr() if pos is not None else None, pbs, B, Hq, Hk, T, D, P, *q.stride()[:3], *k.stride()[:3], _OUT_DTYPES[q.dtype],
                 _OUT_DTYPES[k.dtype], _OUT_DTYPES[cos.dtype])
    _lib.check(rc, "rope_forward")
    rope_counts["fwd_launch"] += 1
    return qo, ko, cos, sin, pos, q, k


def rope_forward(q, k, cos, sin, position_ids=None):
    """-> (q_embed, k_embed) = the eager chain's x * cos[pos] + rotate_half(x) * sin[pos] for q and k, bit for bit, each dense in its
    input's dimension order (the chain's own layout).  q and k have one dtype, or one of them is float32 and the tables are: the results
    are then float32, as the chain's promotion makes them.  q [B, Hq, T, D], k [B, Hk, T, D] with a last stride of 1 are read where they lie
    (any other layout is copied once and counted); cos, sin [P, D] or [1, 1, P, D] in the tensors' dtype or float32; position_ids int64
    [B, T] or [1, T], None: the token index.  One launch on the current stream (fwd_launch)."""
    geom = check_rope(q, k, cos, sin, position_ids, "rope_forward")
    return rope_launch_forward(q, k, cos, sin, position_ids, geom)[:2]


def rope_backward(dq_out, dk_out, cos, sin, position_ids, q_like, k_like, need_dq=True, need_dk=True):
    """-> (dq, dk), the bits of the eager chain's autograd, dense in the dimension order of the forward's q and k; None for the one that
    is not needed (neither read, computed nor stored).  dq_out, dk_out: the gradients of rope_forward's results; q_like, k_like: the
    forward's q and k, or their (shape, strides, dtype) -- no value of q or k is read.  One launch (bwd_launch)."""
    if not (need_dq or need_dk):
        raise ValueError("rope_backward: neither dq nor dk is asked for")
    (qshape, qstr, qdt), (kshape, kstr, kdt) = ((tuple(t.shape), tuple(t.stride()), t.dtype) if isinstance(t, torch.Tensor) else (tuple(t[0]), tuple(t[1]), t[2])
                                                for t in (q_like, k_like))
    lead = dq_out if need_dq else dk_out
    grads = {}
    for name, g, shape, need in (("dq_out", dq_out, qshape, need_dq), ("dk_out", dk_out, kshape, need_dk)):
        if need:
            _row_tensors("rope_backward", **{name: g})
            if tuple(g.shape) != shape or g.dtype != lead.dtype or g.device != lead.device:
                raise ValueError(f"rope_backward: {name} is the gradient of a result: {shape} of {lead.dtype} on {lead.device}, got {tuple(g.shape)} of {g.dtype} on {g.device}")
            grads[name] = g
    if len(qshape) != 4 or len(kshape) != 4 or (kshape[0], kshape[2], kshape[3]) != (qshape[0], qshape[2], qshape[3]) or qshape[3] % 2 or not all(qshape + kshape):
        raise ValueError(f"rope_backward: q and k are non-empty [B, H, T, D] with an even D and equal B, T, D, got {qshape} and {kshape}")
    B, Hq, T, D = qshape
    Hk = kshape[1]
    if qdt not in _OUT_DTYPES or kdt not in _OUT_DTYPES or (qdt != kdt and torch.float32 not in (qdt, kdt)) or lead.dtype != rope_result_dtype(qdt, kdt):
        raise TypeError(f"rope_backward: q of {qdt} and k of {kdt} with gradients of {lead.dtype} are not served")
    check_rope_tables(cos, sin, position_ids, lead, B, T, D, "rope_backward", lead.dtype)
    _prep(lead, "rope_backward")
    gq = _rope_served(dq_out) if need_dq else None
    gk = _rope_served(dk_out) if need_dk else None
    cos, sin = _rope_table(cos, D), _rope_table(sin, D)
    pos, pbs = _rope_positions(position_ids, B)
    dq = torch.empty_strided(qshape, rope_dense_like(qshape, qstr), dtype=qdt, device=lead.device) if need_dq else None
    dk = torch.empty_strided(kshape, rope_dense_like(kshape, kstr), dtype=kdt, device=lead.device) if need_dk else None
    zero3 = (0, 0, 0)
    rc = _launch(lead, _lib.lib().fqr_rope_bwd, gq.data_ptr() if need_dq else None, gk.data_ptr() if need_dk else None,
                 dq.data_ptr() if need_dq else None, dk.data_ptr() if need_dk else None, cos.data_ptr(), sin.data_ptr(),
                 pos.data_ptr() if pos is not None else None, pbs, B, Hq, Hk, T, D, cos.shape[0],
                 *(gq.stride()[:3] if need_dq else zero3), *(gk.stride()[:3] if need_dk else zero3), *qstr[:3], *kstr[:3],
                 _OUT_DTYPES[qdt], _OUT_DTYPES[kdt], _OUT_DTYPES[cos.dtype])
    _lib.check(rc, "rope_backward")
    rope_counts["bwd_launch"] += 1
    return dq, dk


# ---- the softmax chain between the two attention products (the fqs2_ header) ------------------------------------------------
attn_counts = {"fwd_launch": 0, "bwd_launch": 0, "copy_route": 0}


@torch.compiler.assume_constant_result      # Python numbers in, a Python float out: a constant of the graph while compiling
def attn_inv(head_dim=None, scale=None, what="attn_softmax"):
    """-> the fp32 factor the scores are multiplied by, as a Python float: `scale` rounded to fp32, or the fp32 reciprocal of
    (float)sqrt(head_dim), which is what `tensor / math.sqrt(head_dim)` multiplies by on the device.  Exactly one of the two is given."""
    if (head_dim is None) == (scale is None):
        raise TypeError(f"{what}: give head_dim (the scores are divided by sqrt(head_dim)) or scale (they are multiplied by it), and not both")
    if scale is not None:
        if isinstance(scale, bool) or not isinstance(scale, (int, float)):
            raise TypeError(f"{what}: scale is a number, got {type(scale).__name__}")
        return ctypes.c_float(scale).value
    if isinstance(head_dim, bool) or not isinstance(head_dim, int):
        raise TypeError(f"{what}: head_dim is an int, got {type(head_dim).__name__}")
    if head_dim <= 0:
        raise ValueError(f"{what}: head_dim={head_dim} must be positive")
    return ctypes.c_float(1.0 / ctypes.c_float(head_dim ** 0.5).value).value      # the quotient of two floats in double, rounded once: fp32's own


def check_attn_softmax(scores, attention_mask=None, head_dim=None, scale=None, what="attn_softmax"):
    """The argument checks of the attention softmax on types, shapes, dtypes and devices alone (the fake implementations of the compiled
    ops run them too) -> (B, H, T, S, inv): TypeError for a non-tensor, a dtype that is not served (float64), a mask whose dtype is neither
    the scores' nor float32, a head_dim / scale of the wrong type or both or neither of them; ValueError for scores that are not a
    non-empty [B, H, T, S], a mask that is not [B, 1, T, S] or [1, 1, T, S], a head_dim that is not positive, tensors on two devices."""
    _row_tensors(what, scores=scores)
    if attention_mask is not None:
        _row_tensors(what, attention_mask=attention_mask)
    if scores.dtype not in _OUT_DTYPES:
        raise TypeError(f"{what}: scores of dtype {scores.dtype} are not served (float32, bfloat16, float16 are; the arithmetic is fp32 for all three)")
    if attention_mask is not None and attention_mask.dtype not in (scores.dtype, torch.float32):
        raise TypeError(f"{what}: a mask of dtype {attention_mask.dtype} beside scores of {scores.dtype} is not served: the scores' dtype or float32")
    inv = attn_inv(head_dim, scale, what)
    if scores.dim() != 4 or scores.numel() == 0:
        raise ValueError(f"{what}: scores are a non-empty [B, H, T, S], got {tuple(scores.shape)}")
    B, H, T, S = scores.shape
    if attention_mask is not None:
        if attention_mask.dim() != 4 or tuple(attention_mask.shape[1:]) != (1, T, S) or attention_mask.shape[0] not in (1, B):
            raise ValueError(f"{what}: the mask is [{B}, 1, {T}, {S}] or [1, 1, {T}, {S}], got {tuple(attention_mask.shape)}")
        if attention_mask.device != scores.device:
            raise ValueError(f"{what}: scores are on {scores.device}, the mask on {attention_mask.device}")
    return B, H, T, S, inv


def _attn_mask(mask, B, T):
    """-> (mask as the launch reads it or None, batch stride, row stride, dtype code): read where it lies with a last stride of 1, else its
    one counted copy; a batch of size 1 beside B > 1 (or an expanded one) has batch stride 0"""
    if mask is None:
        return None, 0, 0, _lib.DTYPE_F32
    if mask.stride(-1) != 1 and mask.shape[-1] > 1:
        attn_counts["copy_route"] += 1
        mask = mask.contiguous()
    return mask, (mask.stride(0) if mask.shape[0] == B and B > 1 else 0), (mask.stride(2) if T > 1 else 0), _OUT_DTYPES[mask.dtype]


def attn_launch_forward(scores, mask, geom, need_stats=True):
    """attn_softmax_forward behind check_attn_softmax's geometry, for a caller that has run the checks -> (y, stats, scores, mask): the
    scores and the mask as the launch read them (what a backward needs)"""
    B, H, T, S, inv = geom
    _prep(scores, "attn_softmax_forward")
    scores = _row_contig(scores, attn_counts)
    mask, mbs, mrs, mcode = _attn_mask(mask, B, T)
    rows = B * H * T
    y = torch.empty_like(scores)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=scores.device) if need_stats else None
    rc = _launch(scores, _lib.lib().fqs2_attn_softmax_fwd, scores.data_ptr(), mask.data_ptr() if mask is not None else None, y.data_ptr(),
                 stats.data_ptr() if need_stats else None, rows, S, B, H, T, mbs, mrs, inv, _OUT_DTYPES[scores.dtype], mcode)
    _lib.check(rc, "attn_softmax_forward")
    attn_counts["fwd_launch"] += 1
    return y, stats, scores, mask


def attn_softmax_forward(scores, attention_mask=None, head_dim=None, scale=None, need_stats=True):
    """-> (y, stats): y = softmax(max(scores / sqrt(head_dim) + mask, finfo.min), -1, float32) in the scores' dtype with the eager chain's
    roundings in front of the softmax (no clamp without a mask, as the reference), and the fp32 [rows, 2] row maxima and sums the
    backward reads (None with need_stats=False: no buffer, nothing written).  scores [B, H, T, S]; the mask [B, 1, T, S] or [1, 1, T, S]
    in the scores' dtype or float32 (the sum then promotes), read where it lies with a last stride of 1.  One launch (fwd_launch)."""
    geom = check_attn_softmax(scores, attention_mask, head_dim, scale, "attn_softmax_forward")
    return attn_launch_forward(scores, attention_mask, geom, need_stats)[:2]


def attn_softmax_backward(g, scores, attention_mask, stats, head_dim=None, scale=None):
    """-> dx of the scores' shape and dtype: the chain's autograd with its casts and the gradient of torch.max (a tie gets half, an element
    below finfo.min none).  g: the gradient of attn_softmax_forward's y (its shape and dtype); scores, mask, head_dim / scale: the
    forward's; stats: the forward's.  No atomics: two calls give the same bits.  One launch (bwd_launch)."""
    with torch.no_grad():
        B, H, T, S, inv = check_attn_softmax(scores, attention_mask, head_dim, scale, "attn_softmax_backward")
    _prep(scores, "attn_softmax_backward")
    _row_tensors("attn_softmax_backward", g=g)
    if g.dtype != scores.dtype or tuple(g.shape) != tuple(scores.shape) or g.device != scores.device:
        raise ValueError(f"attn_softmax_backward: g is the gradient of y: {tuple(scores.shape)} of {scores.dtype} on {scores.device}, got "
                         f"{tuple(g.shape)} of {g.dtype} on {g.device}")
    rows = B * H * T
    _row_stats("attn_softmax_backward", stats, "stats is attn_softmax_forward's", (rows, 2), scores)
    scores = _row_contig(scores.detach(), attn_counts)
    g = _row_contig(g.detach(), attn_counts)
    mask, mbs, mrs, mcode = _attn_mask(attention_mask, B, T)
    dx = torch.empty_like(scores)
    rc = _launch(scores, _lib.lib().fqs2_attn_softmax_bwd, g.data_ptr(), scores.data_ptr(), mask.data_ptr() if mask is not None else None,
                 stats.data_ptr(), dx.data_ptr(), rows, S, B, H, T, mbs, mrs, inv, _OUT_DTYPES[scores.dtype], mcode)
    _lib.check(rc, "attn_softmax_backward")
    attn_counts["bwd_launch"] += 1
    return dx
