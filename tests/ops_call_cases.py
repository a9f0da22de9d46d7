"""The call log of ops.py's masked STE backwards and N-tensor Sym forwards: what each route hands to the C ABI, and what it gives back.

`record()` runs every case below against the imported package with the launching entry points of `_lib.lib()` shadowed (as LaunchCounter
in test_gpu_layer_fullsize.py does) and returns {case name: log}.  tests/ops_call_log.json is that dict, recorded once at commit a8f632c,
BEFORE the functions' shared per-tensor work moved into ops._mask_slot; test_gpu_ops_call_log.py compares the imported package with it,
cell for cell, and any later change to these functions has to pass it too.
`python tests/ops_call_cases.py OUT.json` writes a recording.

A case's log:
  calls     every launching entry point called, in order, with its arguments: numbers verbatim (so `lo` and `float(lo)` differ when the
            case passes an int clip), None as None, the stream as "stream", struct arrays field by field (fq_rows_view included), and
            every pointer by name: an input of the case (g0, side0+0, side0+40: side buffers always with their byte offset), a tensor
            the ops function returned (out0, y1, side1+24), or a temporary the function made on the way, named after the ATen op that
            made it and what it was made from -- clone(g0), _to_copy(g0), empty_like(g0), empty().  "?" is a pointer that is none of
            these; the test refuses a log that holds one.
  refused   entry points the recorder answered FQ_ERR_UNSUPPORTED for, without launching (the fall-back arms)
  returns   per returned tensor dtype, shape, strides, data_ptr() % 16, which input it IS, and a SHA-256 of its bytes (of a side
            buffer: its bounds half only -- rows that cannot clip leave their bitmap words unwritten); ints and None as they are
  raises    exception type and message (a message of _lib.check() up to its "(code N)": what follows is the library's last-error
            text, which a refusal made by the recorder does not set)
  views     by how much ops._view_served()'s counter went up

Arm -> case (the functions as recorded; `*` stands for the dtype / in-place variants of the name):
  train_backward         _prep refusal: train_backward/int32, /cpu; strided attempt served: */cols; attempt refused by the layout
                         (rows_view False): */t; by alignment: */cols_off; by the library (recorder): */cols/refused-v; _aligned's clone:
                         */offset; in place: */inplace; rows == 0 (the launch returns at once): */empty; the library's refusal raises:
                         train_backward/width100 and */refused
  train_backward_wide    out_dtype without a code: train_backward_wide/out-int32; strided fp32 gradient served: */cols; bf16 gradient
                         (.float(), and no strided attempt although its rows are strided): */bf16-grad, */bf16-grad-cols; refusal raises:
                         */width100, */refused
  ste_backward_mask      _prep refusal: ste_backward_mask/cpu; numel() == 0 returns before the launch: */empty; no strided attempt: */cols
                         takes the copy; refusal raises: */refused; float(lo): */int-clip (train_backward/int-clip passes the int)
  pair_backward          left / right None -> train_backward: */gw-none, */gx-none (with inplace_w: the x side never in place); strided
                         attempt: */w-cols, */x-cols; attempt refused -> copy path: */x-t, */x-cols/refused-v; refused pair -> two
                         fq_ste_bwd_mask on the ALIGNED tensors: */refused, */offset/refused
  pair_backward_wide     None arms -> train_backward_wide; no strided attempt (*/x-cols copies); .float() per operand: */bf16-gw;
                         refusal raises: */refused
  multi_backward         no live gradient: multi_backward/none-live; exactly one -> train_backward: */one-live; 2, 3, 4 live, holes, an
                         inplace list; refused -> one fq_ste_bwd_mask per live tensor: */refused; a strided member is copied: */strided
  _mask_backward_v       reached through the strided cases above (1 and 2 tensors, in place or not, wide or not); `ov is False` behind
                         _strided_out is unreachable: empty_like gives a result either the gradient's own (dense) strides, whose rows_view
                         the gradient has just passed, or contiguous ones
  pair_forward           need_w x need_x, contiguous / strided, autocast off / narrow / wide, autocast dtype != operand dtype, refused
                         (both entry points), and the ineligible inputs by name: pair_forward/ineligible/*; `wqv is False` behind
                         _strided_out is unreachable for the reason above
  multi_forward          2, 3, 4 tensors with mixed need, autocast on / off / other dtype, refused, multi_forward/ineligible/*
"""
import ctypes
import hashlib
import json
import os
import sys
import zlib

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ENTRIES = ("fq_sym_fwd_pair", "fq_sym_fwd_multi", "fq_sym_fwd_multi_v",
           "fq_ste_bwd_mask", "fq_ste_bwd_mask_pair", "fq_ste_bwd_mask_wide", "fq_ste_bwd_mask_multi", "fq_ste_bwd_mask_multi_v",
           "fq_sym_fwd_train", "fq_asym_fwd_train", "fq_rowwise_fwd_v", "fq_sym_fwd_autocast")
LOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ops_call_log.json")
LO, HI = -2.0, 2.0
COLS = 256
BF16, F32 = torch.bfloat16, torch.float32
SHORT = {torch.bfloat16: "bf16", torch.float32: "fp32"}


def _extent(t):
    """bytes from t.data_ptr() to the end of its last element"""
    if not t.numel():
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


class _Made(TorchDispatchMode):
    """every CUDA tensor an ATen op returns while a case runs (kept alive, so no address is handed out twice)"""

    def __init__(self):
        super().__init__()
        self.made = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if isinstance(out, torch.Tensor) and out.is_cuda and out.numel():
            src = next((a for a in args if isinstance(a, torch.Tensor)), None)
            self.made.append((func.overloadpacket.__name__, src, out))
        return out


class Recorder:
    """shadows ENTRIES on the loaded library; while a case runs, logs each call and refuses the entry points named in `refuse`"""

    def __init__(self):
        from llm_qat_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.calls, self.refuse = None, ()

    def __enter__(self):
        self.orig = {}
        for name in ENTRIES:
            f = getattr(self.L, name)
            self.orig[name] = f
            setattr(self.L, name, self._shadow(name, f))
        return self

    def __exit__(self, *exc):
        for name, f in self.orig.items():
            setattr(self.L, name, f)

    def _shadow(self, name, f):
        def g(*a):
            if self.calls is None:
                return f(*a)
            assert len(a) == len(f.argtypes), (name, len(a))
            self.calls.append([name, [_raw(v, t) for v, t in zip(a[:-1], f.argtypes)] + ["stream"]])
            if name in self.refuse:
                return self._lib.ERR_UNSUPPORTED
            return f(*a)
        return g


def _raw(v, ctype):
    """one argument as plain data; pointers as {"ptr": address} until the case's tensors are known"""
    if ctype is ctypes.c_void_p:
        return None if v is None else {"ptr": int(v)}
    target = getattr(ctype, "_type_", None)
    if isinstance(target, type) and issubclass(target, ctypes.Structure):
        if isinstance(v, ctypes.Array):
            return [_raw_struct(v[i]) for i in range(len(v))]
        return None if v is None else _raw_struct(v)
    if v is None or type(v) in (int, float, bool):
        return v
    return f"{type(v).__name__}:{v!r}"


def _raw_struct(s):
    out = {}
    for fname, ftype in s._fields_:
        v = getattr(s, fname)
        if ftype is ctypes.c_void_p:
            out[fname] = None if v is None else {"ptr": int(v)}
        elif issubclass(ftype, ctypes.Structure):
            out[fname] = _raw_struct(v)
        else:
            out[fname] = v
    return out


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest() if t.numel() else "empty"


class Case:
    """one case: name its inputs with inp(), then run() one ops function"""

    def __init__(self, rec, name):
        self.rec, self.name = rec, name
        self.gen = torch.Generator(device="cpu").manual_seed(zlib.crc32(name.encode()))
        self.inputs = []      # (name, tensor)
        self.log = None

    def randn(self, *shape, dtype=BF16, scale=1.0):
        return (torch.randn(*shape, generator=self.gen) * scale).to(dtype).cuda()

    def inp(self, name, t):
        self.inputs.append((name, t))
        return t

    def run(self, fn, *args, refuse=(), autocast=None, **kw):
        from llm_qat_amd import ops
        rec, made = self.rec, _Made()
        rec.calls, rec.refuse = [], tuple(refuse)
        served0, res, raised = ops._views_served, None, None
        try:
            with made:
                if autocast is None:
                    res = getattr(ops, fn)(*args, **kw)
                else:
                    with torch.autocast("cuda", dtype=autocast):
                        res = getattr(ops, fn)(*args, **kw)
        except Exception as e:  # noqa: BLE001 -- the exception is what the case logs
            raised = {"type": type(e).__name__, "message": str(e).split("): ")[0] + ")" if " failed (code " in str(e) else str(e)}
        finally:
            calls, rec.calls, rec.refuse = rec.calls, None, ()
        torch.cuda.synchronize()
        outs, extra = _label(fn, res)
        ranges = [(n, t) for n, t in self.inputs] + [(n, t) for n, t in outs if isinstance(t, torch.Tensor)]
        known = [(n, t.data_ptr(), t.data_ptr() + _extent(t)) for n, t in ranges if t.is_cuda and t.numel()]

        def name_of(p):
            if p == 0:      # the data_ptr() of a tensor without elements
                return "0"
            for n, a, b in known:
                if a <= p < b:
                    return f"{n}+{p - a}" if p != a or n.startswith("side") else n
            return "?"
        for op, src, out in made.made:   # temporaries, in the order they were made: named after the op and its first tensor argument
            if name_of(out.data_ptr()) == "?":
                s = name_of(src.data_ptr()) if src is not None and src.is_cuda and src.numel() else ""
                known.append((f"{op}({s})", out.data_ptr(), out.data_ptr() + _extent(out)))

        def resolve(v):
            if isinstance(v, dict):
                return name_of(v["ptr"]) if set(v) == {"ptr"} else {k: resolve(x) for k, x in v.items()}
            return [resolve(x) for x in v] if isinstance(v, list) else v
        returns = None
        if res is not None:
            returns = dict(extra)
            for n, t in outs:
                if not isinstance(t, torch.Tensor):
                    returns[n] = t
                    continue
                rows = extra["rows"][int(n[4:])] if n.startswith("side") else None
                returns[n] = {"dtype": str(t.dtype), "shape": list(t.shape), "strides": list(t.stride()), "align": t.data_ptr() % 16,
                              "is": next((m for m, i in self.inputs if i is t), None),
                              "sha": _sha(t if rows is None else t[:rows * 8])}
        self.log = {"calls": resolve(calls), "refused": list(refuse), "returns": returns, "raises": raised,
                    "views": ops._views_served - served0}


def _label(fn, res):
    """-> ([(name, returned value)], {what else the function returned})"""
    if res is None:
        return [], {}
    if fn == "pair_forward":
        return list(zip(("y0", "y1", "side0", "side1"), res[:4])), {"type": type(res).__name__, "rows": list(res[4:6]), "cols": res[6]}
    if fn == "multi_forward":
        ys, sides, rows, cols = res
        return ([(f"y{i}", y) for i, y in enumerate(ys)] + [(f"side{i}", s) for i, s in enumerate(sides)],
                {"type": [type(res).__name__, type(ys).__name__, type(sides).__name__, type(rows).__name__], "rows": list(rows), "cols": cols})
    seq = res if isinstance(res, (list, tuple)) else [res]
    return [(f"out{i}", t) for i, t in enumerate(seq)], {"type": type(res).__name__}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("contig", "offset", "cols", "cols_off", "t")


def tensor(c, rows, dtype, layout="contig", cols=COLS, scale=1.0):
    """[rows, cols] in one of the layouts: contiguous; contiguous at an address that is no multiple of 16; strided rows the kernels serve
    (a column slice of a tensor twice as wide); the same at a misaligned address; a transpose (rows_view refuses it)"""
    if layout == "contig":
        return c.randn(rows, cols, dtype=dtype, scale=scale)
    if layout == "offset":
        t = c.randn(rows * cols + 1, dtype=dtype, scale=scale)[1:].view(rows, cols)
        assert t.is_contiguous() and t.data_ptr() & 15
        return t
    if layout == "cols":
        return c.randn(rows, 2 * cols, dtype=dtype, scale=scale)[:, :cols]
    if layout == "cols_off":
        return c.randn(rows, 2 * cols, dtype=dtype, scale=scale)[:, 1:cols + 1]
    assert layout == "t", layout
    return c.randn(cols, rows, dtype=dtype, scale=scale).t()


def side_of(c, rows, dtype, wide=False, cols=COLS):
    """the side buffer of a training forward over a fresh [rows, cols] operand, some of whose elements lie beyond the clip"""
    from llm_qat_amd import ops
    x = c.randn(rows, cols, dtype=dtype, scale=1.5)
    if wide:
        with torch.autocast("cuda", dtype=dtype):
            _, side, r, _, got = ops.sym_forward_autocast(x, 8, False, wide=True, lo=LO, hi=HI, train="mask")
        assert got == "mask"
    else:
        _, side, r, _ = ops.train_forward("sym", x, 8, False, LO, HI)
    assert r == rows
    return side


def dummy_side(c, nbytes=256):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def single_backward_cases(add):
    for dt in (BF16, F32):
        for layout in LAYOUTS:
            for inplace in (False, True):
                tag = f"{SHORT[dt]}/{layout}" + ("/inplace" if inplace else "")

                def tb(c, dt=dt, layout=layout, inplace=inplace):
                    g, side = c.inp("g0", tensor(c, 5, dt, layout)), c.inp("side0", side_of(c, 5, dt))
                    c.run("train_backward", g, side, 5, COLS, LO, HI, inplace=inplace)
                add(f"train_backward/{tag}", tb)

                def sm(c, dt=dt, layout=layout, inplace=inplace):
                    from llm_qat_amd import ops
                    g, side = c.inp("g0", tensor(c, 5, dt, layout)), c.inp("side0", side_of(c, 5, dt))
                    bounds, mask = ops.split_side(side, 5)
                    c.run("ste_backward_mask", g, LO, HI, bounds, mask, 5, COLS, inplace=inplace)
                add(f"ste_backward_mask/{tag}", sm)
    for layout in LAYOUTS:          # wide: bf16 operands, fp32 gradients, inside autocast(bf16)
        def tw(c, layout=layout):
            g, side = c.inp("g0", tensor(c, 5, F32, layout)), c.inp("side0", side_of(c, 5, BF16, wide=True))
            c.run("train_backward_wide", g, side, 5, COLS, LO, HI, BF16, autocast=BF16)
        add(f"train_backward_wide/{layout}", tw)
    for layout in ("contig", "cols", "t"):      # a bf16 gradient behind a wide forward: the .float() arm
        def twb(c, layout=layout):
            g, side = c.inp("g0", tensor(c, 5, BF16, layout)), c.inp("side0", side_of(c, 5, BF16, wide=True))
            c.run("train_backward_wide", g, side, 5, COLS, LO, HI, BF16, autocast=BF16)
        add("train_backward_wide/bf16-grad" + ("" if layout == "contig" else f"-{layout}"), twb)

    def empty(fn, inplace=False):
        def run(c):
            g, side = c.inp("g0", torch.empty(0, COLS, dtype=F32 if fn == "train_backward_wide" else BF16, device="cuda")), c.inp("side0", dummy_side(c))
            if fn == "train_backward":
                c.run(fn, g, side, 0, COLS, LO, HI, inplace=inplace)
            elif fn == "train_backward_wide":
                c.run(fn, g, side, 0, COLS, LO, HI, BF16, autocast=BF16)
            else:
                c.run(fn, g, LO, HI, side[:0].view(F32).view(0, 2), side, 0, COLS, inplace=inplace)
        return run
    for fn in ("train_backward", "train_backward_wide", "ste_backward_mask"):
        add(f"{fn}/empty", empty(fn))
        if fn != "train_backward_wide":
            add(f"{fn}/empty/inplace", empty(fn, True))

    # what the functions refuse themselves
    def bad_input(fn, g_of, **kw):
        def run(c):
            g, side = g_of(c), c.inp("side0", dummy_side(c))
            if fn == "ste_backward_mask":
                c.run(fn, g, LO, HI, side[:40].view(F32).view(5, 2), side[40:], 5, COLS)
            elif fn == "train_backward_wide":
                c.run(fn, g, side, 5, COLS, LO, HI, kw["out_dtype"], autocast=BF16)
            else:
                c.run(fn, g, side, 5, COLS, LO, HI)
        return run
    add("train_backward/int32", bad_input("train_backward", lambda c: c.inp("g0", torch.ones(5, COLS, dtype=torch.int32, device="cuda"))))
    add("train_backward/cpu", bad_input("train_backward", lambda c: torch.ones(5, COLS, dtype=BF16)))
    add("ste_backward_mask/int32", bad_input("ste_backward_mask", lambda c: c.inp("g0", torch.ones(5, COLS, dtype=torch.int32, device="cuda"))))
    add("ste_backward_mask/cpu", bad_input("ste_backward_mask", lambda c: torch.ones(5, COLS, dtype=BF16)))
    add("train_backward_wide/out-int32", bad_input("train_backward_wide", lambda c: c.inp("g0", tensor(c, 5, F32)), out_dtype=torch.int32))
    add("train_backward_wide/cpu", bad_input("train_backward_wide", lambda c: torch.ones(5, COLS), out_dtype=BF16))

    # refusals: by the library itself (a row length the mask path does not serve: refused before anything is launched) and by the recorder
    def width100(fn):
        def run(c):
            from llm_qat_amd import ops
            assert ops._mask_bytes(2, 100, ops._DTYPES[BF16]) == 0
            g, side = c.inp("g0", tensor(c, 2, F32 if fn == "train_backward_wide" else BF16, cols=100)), c.inp("side0", dummy_side(c))
            if fn == "ste_backward_mask":
                c.run(fn, g, LO, HI, side[:16].view(F32).view(2, 2), side[16:], 2, 100)
            elif fn == "train_backward_wide":
                c.run(fn, g, side, 2, 100, LO, HI, BF16, autocast=BF16)
            else:
                c.run(fn, g, side, 2, 100, LO, HI)
        return run

    def refused(fn, layout, refuse, int_clip=False):
        def run(c):
            from llm_qat_amd import ops
            wide = fn == "train_backward_wide"
            g, side = c.inp("g0", tensor(c, 5, F32 if wide else BF16, layout)), c.inp("side0", side_of(c, 5, BF16, wide=wide))
            lo, hi = (-2, 2) if int_clip else (LO, HI)
            if fn == "ste_backward_mask":
                bounds, mask = ops.split_side(side, 5)
                c.run(fn, g, lo, hi, bounds, mask, 5, COLS, refuse=refuse)
            elif wide:
                c.run(fn, g, side, 5, COLS, lo, hi, BF16, refuse=refuse, autocast=BF16)
            else:
                c.run(fn, g, side, 5, COLS, lo, hi, refuse=refuse)
        return run
    for fn, entry in (("train_backward", "fq_ste_bwd_mask"), ("train_backward_wide", "fq_ste_bwd_mask_wide"), ("ste_backward_mask", "fq_ste_bwd_mask")):
        add(f"{fn}/width100", width100(fn))
        add(f"{fn}/refused", refused(fn, "contig", (entry,)))
        add(f"{fn}/int-clip", refused(fn, "contig", (), int_clip=True))
        add(f"{fn}/cols/int-clip", refused(fn, "cols", (), int_clip=True))
        if fn != "ste_backward_mask":
            add(f"{fn}/cols/refused-v", refused(fn, "cols", ("fq_ste_bwd_mask_multi_v",)))


def pair_backward_cases(add):
    def pair(wide, dt, live, lw, lx, inplace_w=False, refuse=(), gdt=None, int_clip=False):
        def run(c):
            gdt_w, gdt_x = gdt or ((F32, F32) if wide else (dt, dt))
            gw = c.inp("g0", tensor(c, 3, gdt_w, lw)) if live[0] else None
            gx = c.inp("g1", tensor(c, 5, gdt_x, lx)) if live[1] else None
            sw, sx = c.inp("side0", side_of(c, 3, dt, wide=wide)), c.inp("side1", side_of(c, 5, dt, wide=wide))
            lo, hi = (-2, 2) if int_clip else (LO, HI)
            if wide:
                c.run("pair_backward_wide", gw, gx, sw, sx, 3, 5, COLS, lo, hi, dt, refuse=refuse, autocast=dt)
            else:
                c.run("pair_backward", gw, gx, sw, sx, 3, 5, COLS, lo, hi, inplace_w=inplace_w, refuse=refuse)
        return run
    lives = (("both", (1, 1)), ("gw-none", (0, 1)), ("gx-none", (1, 0)))
    for ln, live in lives:
        for layouts in (("contig", "contig"), ("cols", "contig"), ("contig", "cols")):
            lay = {("contig", "contig"): "contig", ("cols", "contig"): "w-cols", ("contig", "cols"): "x-cols"}[layouts]
            for inplace_w in (False, True):
                for dt in (BF16, F32):
                    add(f"pair_backward/{SHORT[dt]}/{ln}/{lay}" + ("/inplace" if inplace_w else ""), pair(False, dt, live, *layouts, inplace_w=inplace_w))
            add(f"pair_backward_wide/{ln}/{lay}", pair(True, BF16, live, *layouts))
        for inplace_w in (False, True):
            tag = f"pair_backward/bf16/{ln}/contig" + ("/inplace" if inplace_w else "")
            add(tag + "/refused", pair(False, BF16, live, "contig", "contig", inplace_w=inplace_w, refuse=("fq_ste_bwd_mask_pair",)))
        add(f"pair_backward_wide/{ln}/contig/refused", pair(True, BF16, live, "contig", "contig", refuse=("fq_ste_bwd_mask_wide",)))
    for inplace_w in (False, True):
        tag = "/inplace" if inplace_w else ""
        add("pair_backward/bf16/both/offset" + tag, pair(False, BF16, (1, 1), "offset", "offset", inplace_w=inplace_w))
        add("pair_backward/bf16/both/offset/refused" + tag, pair(False, BF16, (1, 1), "offset", "contig", inplace_w=inplace_w, refuse=("fq_ste_bwd_mask_pair",)))
        add("pair_backward/bf16/both/x-t" + tag, pair(False, BF16, (1, 1), "contig", "t", inplace_w=inplace_w))
        add("pair_backward/bf16/both/w-cols_off" + tag, pair(False, BF16, (1, 1), "cols_off", "contig", inplace_w=inplace_w))
        add("pair_backward/bf16/both/both-cols" + tag, pair(False, BF16, (1, 1), "cols", "cols", inplace_w=inplace_w))
        add("pair_backward/bf16/both/x-cols/refused-v" + tag, pair(False, BF16, (1, 1), "contig", "cols", inplace_w=inplace_w, refuse=("fq_ste_bwd_mask_multi_v",)))
    add("pair_backward/bf16/both/contig/int-clip", pair(False, BF16, (1, 1), "contig", "contig", int_clip=True))
    add("pair_backward/bf16/both/x-cols/int-clip", pair(False, BF16, (1, 1), "contig", "cols", int_clip=True))
    add("pair_backward/bf16/both/contig/refused/int-clip", pair(False, BF16, (1, 1), "contig", "contig", refuse=("fq_ste_bwd_mask_pair",), int_clip=True))
    add("pair_backward_wide/both/contig/int-clip", pair(True, BF16, (1, 1), "contig", "contig", int_clip=True))
    add("pair_backward_wide/both/offset", pair(True, BF16, (1, 1), "offset", "offset"))
    add("pair_backward_wide/both/bf16-gw", pair(True, BF16, (1, 1), "contig", "contig", gdt=(BF16, F32)))
    add("pair_backward_wide/both/bf16-gx-t", pair(True, BF16, (1, 1), "contig", "t", gdt=(F32, BF16)))
    add("pair_backward_wide/gx-none/bf16-gw", pair(True, BF16, (1, 0), "contig", "contig", gdt=(BF16, F32)))


MULTI_ROWS = (5, 3, 2, 1)


def multi_backward_cases(add):
    def multi(n, live, dt=BF16, inplace=None, refuse=(), layouts=None, int_clip=False):
        def run(c):
            grads = [c.inp(f"g{i}", tensor(c, MULTI_ROWS[i], dt, (layouts or {}).get(i, "contig"))) if live[i] else None for i in range(n)]
            sides = [c.inp(f"side{i}", side_of(c, MULTI_ROWS[i], dt)) for i in range(n)]
            lo, hi = (-2, 2) if int_clip else (LO, HI)
            kw = {} if inplace is None else {"inplace": inplace}
            c.run("multi_backward", grads, sides, list(MULTI_ROWS[:n]), COLS, lo, hi, refuse=refuse, **kw)
        return run
    for dt in (BF16, F32):
        for n in (2, 3, 4):
            add(f"multi_backward/{SHORT[dt]}/{n}", multi(n, [1] * n, dt))
    add("multi_backward/none-live", multi(3, [0, 0, 0]))
    add("multi_backward/one-live", multi(3, [0, 1, 0]))
    add("multi_backward/one-live/inplace", multi(3, [0, 0, 1], inplace=[False, False, True]))
    add("multi_backward/one-live/cols", multi(2, [0, 1], layouts={1: "cols"}))
    add("multi_backward/holes-3", multi(3, [1, 0, 1]))
    add("multi_backward/holes-4", multi(4, [0, 1, 1, 1]))
    add("multi_backward/holes-4/inplace", multi(4, [1, 0, 1, 1], inplace=[True, True, False, True]))
    add("multi_backward/3/inplace", multi(3, [1, 1, 1], inplace=[True, False, True]))
    add("multi_backward/4/refused", multi(4, [1, 1, 1, 1], refuse=("fq_ste_bwd_mask_multi",)))
    add("multi_backward/holes-3/inplace/refused", multi(3, [1, 0, 1], inplace=[True, False, False], refuse=("fq_ste_bwd_mask_multi",)))
    add("multi_backward/3/refused/int-clip", multi(3, [1, 1, 1], refuse=("fq_ste_bwd_mask_multi",), int_clip=True))
    add("multi_backward/3/strided", multi(3, [1, 1, 1], layouts={0: "cols", 2: "offset"}))
    add("multi_backward/3/strided/inplace", multi(3, [1, 1, 1], layouts={0: "cols", 1: "t", 2: "offset"}, inplace=[True, True, True]))
    add("multi_backward/2/int-clip", multi(2, [1, 1], int_clip=True))


def pair_forward_cases(add):
    def pf(dt, need, lw="contig", lx="contig", autocast=None, wide=None, refuse=(), shapes=None, int_clip=False):
        def run(c):
            (sw, sx) = shapes or ((3, COLS), (5, COLS))
            w = c.inp("x0", tensor(c, sw[0], dt, lw, cols=sw[1], scale=1.5)) if not callable(sw) else c.inp("x0", sw(c))
            x = c.inp("x1", tensor(c, sx[0], dt, lx, cols=sx[1], scale=1.5)) if not callable(sx) else c.inp("x1", sx(c))
            lo, hi = (-2, 2) if int_clip else (LO, HI)
            kw = {} if wide is None else {"wide": wide}
            c.run("pair_forward", w, x, 4, 8, lo, hi, need[0], need[1], refuse=refuse, autocast=autocast, **kw)
        return run
    for need in ((True, True), (True, False), (False, True), (False, False)):
        nt = "need-" + "".join("wx"[i] for i in range(2) if need[i]) if any(need) else "need-none"
        for lay, (lw, lx) in (("contig", ("contig", "contig")), ("w-cols", ("cols", "contig")), ("x-cols", ("contig", "cols"))):
            for dt in (BF16, F32):
                add(f"pair_forward/{SHORT[dt]}/{nt}/{lay}", pf(dt, need, lw, lx))
            add(f"pair_forward/autocast-narrow/{nt}/{lay}", pf(BF16, need, lw, lx, autocast=BF16))
            add(f"pair_forward/autocast-wide/{nt}/{lay}", pf(BF16, need, lw, lx, autocast=BF16, wide=True))
    add("pair_forward/bf16/wide-outside-autocast", pf(BF16, (True, True), wide=True))
    add("pair_forward/fp32/inside-autocast", pf(F32, (True, True), autocast=BF16, wide=True))
    add("pair_forward/autocast-other-dtype", pf(BF16, (True, True), autocast=torch.float16))
    add("pair_forward/autocast-other-dtype/wide", pf(BF16, (True, True), autocast=torch.float16, wide=True))
    add("pair_forward/bf16/int-clip", pf(BF16, (True, True), int_clip=True))
    add("pair_forward/bf16/x-cols/int-clip", pf(BF16, (True, True), lx="cols", int_clip=True))
    add("pair_forward/bf16/refused", pf(BF16, (True, True), refuse=("fq_sym_fwd_pair",)))
    add("pair_forward/bf16/x-cols/refused", pf(BF16, (True, True), lx="cols", refuse=("fq_sym_fwd_multi_v",)))
    add("pair_forward/bf16/offset", pf(BF16, (True, True), lw="offset"))        # the library refuses the alignment itself
    add("pair_forward/bf16/3d", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(2, 3, COLS, scale=1.5))))
    add("pair_forward/bf16/3d-transposed", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(3, 2, COLS, scale=1.5).transpose(0, 1))))
    add("pair_forward/bf16/1d", pf(BF16, (True, True), shapes=(lambda c: c.randn(COLS), (5, COLS))))
    # not eligible: None, and nothing is called
    inel = "pair_forward/ineligible/"
    add(inel + "dtype", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(5, COLS, dtype=F32))))
    add(inel + "cpu", pf(BF16, (True, True), shapes=(lambda c: torch.ones(3, COLS, dtype=BF16), lambda c: torch.ones(5, COLS, dtype=BF16))))
    add(inel + "device", pf(BF16, (True, True), shapes=((3, COLS), lambda c: torch.ones(5, COLS, dtype=BF16))))
    add(inel + "int32", pf(BF16, (True, True), shapes=(lambda c: torch.ones(3, COLS, dtype=torch.int32, device="cuda"),
                                                      lambda c: torch.ones(5, COLS, dtype=torch.int32, device="cuda"))))
    add(inel + "last-dim", pf(BF16, (True, True), shapes=((3, COLS), (5, 2 * COLS))))
    add(inel + "empty-x", pf(BF16, (True, True), shapes=((3, COLS), (0, COLS))))
    add(inel + "empty-w", pf(BF16, (True, True), shapes=((0, COLS), (5, COLS))))
    add(inel + "width100", pf(BF16, (True, True), shapes=((3, 100), (5, 100))))
    add(inel + "4d", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(1, 2, 3, COLS))))
    add(inel + "4d-strided", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(1, 2, 3, 2 * COLS)[..., :COLS])))
    add(inel + "0d", pf(BF16, (True, True), shapes=((3, COLS), lambda c: c.randn(1)[0])))
    add(inel + "transposed", pf(BF16, (True, True), lx="t"))


def multi_forward_cases(add):
    def mf(n, need, dt=BF16, autocast=None, refuse=(), swap=None, int_clip=False, bits=(8, 4, 4, 4)):
        def run(c):
            ts = [tensor(c, MULTI_ROWS[i % 4], dt, scale=1.5) for i in range(n)]
            for i, t in (swap(c) if swap else {}).items():
                ts[i] = t
            for i, t in enumerate(ts):
                c.inp(f"x{i}", t)
            lo, hi = (-2, 2) if int_clip else (LO, HI)
            c.run("multi_forward", ts, [bits[i % 4] for i in range(n)], list(need), lo, hi, refuse=refuse, autocast=autocast)
        return run
    for dt in (BF16, F32):
        add(f"multi_forward/{SHORT[dt]}/2", mf(2, (True, False), dt))
        add(f"multi_forward/{SHORT[dt]}/3", mf(3, (True, True, False), dt))
        add(f"multi_forward/{SHORT[dt]}/4", mf(4, (False, True, False, True), dt))
    add("multi_forward/bf16/4/need-all", mf(4, (True,) * 4))
    add("multi_forward/bf16/3/need-none", mf(3, (False,) * 3))
    add("multi_forward/autocast/2", mf(2, (True, True), autocast=BF16))
    add("multi_forward/autocast/4", mf(4, (True, False, True, False), autocast=BF16))
    add("multi_forward/autocast/fp32-tensors", mf(3, (True,) * 3, F32, autocast=BF16))
    add("multi_forward/autocast-other-dtype", mf(3, (True,) * 3, autocast=torch.float16))
    add("multi_forward/bf16/3/refused", mf(3, (True,) * 3, refuse=("fq_sym_fwd_multi",)))
    add("multi_forward/bf16/3/int-clip", mf(3, (True,) * 3, int_clip=True))
    add("multi_forward/bf16/3/float-bits", mf(3, (True,) * 3, bits=(8.0, 4.0, 4.0, 4.0)))
    add("multi_forward/bf16/3d-member", mf(3, (True,) * 3, swap=lambda c: {1: c.randn(2, 3, COLS, scale=1.5)}))
    add("multi_forward/bf16/offset-member", mf(3, (True,) * 3, swap=lambda c: {1: tensor(c, 3, BF16, "offset")}))   # refused by the library
    inel = "multi_forward/ineligible/"
    add(inel + "1-tensor", mf(1, (True,)))
    add(inel + "5-tensors", mf(5, (True,) * 5))
    add(inel + "strided-member", mf(3, (True,) * 3, swap=lambda c: {2: tensor(c, 2, BF16, "cols")}))
    add(inel + "strided-first", mf(3, (True,) * 3, swap=lambda c: {0: tensor(c, 5, BF16, "cols")}))
    add(inel + "width", mf(3, (True,) * 3, swap=lambda c: {1: tensor(c, 3, BF16, cols=2 * COLS)}))
    add(inel + "width100", mf(2, (True,) * 2, swap=lambda c: {0: tensor(c, 5, BF16, cols=100), 1: tensor(c, 3, BF16, cols=100)}))
    add(inel + "member-dtype", mf(3, (True,) * 3, swap=lambda c: {1: tensor(c, 3, F32)}))
    add(inel + "int32", mf(2, (True,) * 2, swap=lambda c: {i: torch.ones(3, COLS, dtype=torch.int32, device="cuda") for i in range(2)}))
    add(inel + "cpu", mf(2, (True,) * 2, swap=lambda c: {i: torch.ones(3, COLS, dtype=BF16) for i in range(2)}))
    add(inel + "member-device", mf(2, (True,) * 2, swap=lambda c: {1: torch.ones(3, COLS, dtype=BF16)}))
    add(inel + "empty-member", mf(3, (True,) * 3, swap=lambda c: {2: tensor(c, 0, BF16)}))
    add(inel + "4d-member", mf(3, (True,) * 3, swap=lambda c: {1: c.randn(1, 1, 3, COLS)}))


def cases():
    out = []

    def add(name, fn):
        assert name not in dict(out), name
        out.append((name, fn))
    for family in (single_backward_cases, pair_backward_cases, multi_backward_cases, pair_forward_cases, multi_forward_cases):
        family(add)
    return out


def record():
    """-> {case name: log} of the imported package, in the session semantics the suite runs under ("cpu_eager")"""
    import llm_qat_amd
    sem = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    logs = {}
    try:
        with Recorder() as rec:
            for name, fn in cases():
                c = Case(rec, name)
                fn(c)
                assert c.log is not None, name
                logs[name] = c.log
    finally:
        llm_qat_amd.set_semantics(sem)
    return logs


def dump(logs, path):
    """one case per line, so that a difference reads as a line"""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in logs.items()) + "\n}\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump(record(), sys.argv[1])
    print("recorded", len(cases()), "cases ->", sys.argv[1])
