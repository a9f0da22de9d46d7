"""CPU tier of the MX front-end's shared helpers (ops._mx_quantize / _mx_input / _mx_launch, mx_quant._mx_check / _mx_apply, the fake
implementations and dispatchers of compiled.py): what a caller sees of them without a GPU.

1. The refusal table: which exception, with which message, every combination of good and faulty arguments gives -- so also which of two
   simultaneous faults answers, which is the order of the checks.  TABLE was recorded by running the commit before the helpers were
   folded (observe() below, on that commit's package); the test asks the same of the code as it is, cell for cell.
2. The dispatch tables: which custom op each combination of options reaches while compiling, and with which arguments.
3. The fake implementations, on meta tensors: shapes, dtypes and messages."""
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import compiled, mx_quant, ops
from llm_qat_amd import utils_quant as U

BAD_FMT, BAD_RULE, BAD_AXIS = "mxfp5", "up", 5
NOT_A_TENSOR = [1.0]


# ---- 1. the refusal table --------------------------------------------------------------------------------------------------------------------
# Every function's cells are a grid: one row per (x, format, axis, shape), one column per (rule, ste / return_mask, rotate).  A good cell on
# a CPU tensor ends at the device check, the last one.

def _quantize_shape(axis, good):
    """the shape that is good / bad for the axis: 64 down a good axis (whole rotation runs too), 48 down a bad one"""
    if axis == -2:
        return (64, 64) if good else (48, 64)
    return (64, 64) if good else (64, 48)


def _quantize_grid(f, fifth_name, fifth_values):
    rows = [(xk, fmt, axis, good) for xk in ("cpu", "obj") for fmt in ("mxfp4", BAD_FMT) for axis in (-1, -2, BAD_AXIS)
            for good in ((True, False) if xk == "cpu" else (True,))]
    cols = [(rule, fifth, rotate) for rule in ("ceil", BAD_RULE) for fifth in fifth_values for rotate in (False, True)]

    def call(row, col):
        xk, fmt, axis, good = row
        rule, fifth, rotate = col
        x = torch.zeros(_quantize_shape(axis, good)) if xk == "cpu" else NOT_A_TENSOR
        return f(x, fmt, rotate=rotate, scale_rule=rule, axis=axis, **{fifth_name: fifth})
    return rows, cols, call


def _export_grid():
    rows = [(xk, fmt, shape) for xk in ("cpu", "obj") for fmt in ("mxfp4", "mxfp6_e2m3", BAD_FMT)
            for shape in (((2, 64), (2, 32), (2, 48)) if xk == "cpu" else ((2, 64),))]      # good; no whole rotation run; no whole block
    cols = [(rule, rotate) for rule in ("ceil", BAD_RULE) for rotate in (False, True)]

    def call(row, col):
        xk, fmt, shape = row
        return ops.mx_export(torch.zeros(shape) if xk == "cpu" else NOT_A_TENSOR, fmt, rotate=col[1], scale_rule=col[0])
    return rows, cols, call


def _ste_grid():
    rows = [(2, 64), (2, 32), (2, 48), None]                                                  # the gradient's shape; None: not a tensor
    cols = [(mask, rotate) for mask in ("good", "dtype", "size", "obj") for rotate in (False, True)]

    def call(row, col):
        g = NOT_A_TENSOR if row is None else torch.zeros(row)
        n = 128 if row is None else g.numel()
        mask = {"good": torch.zeros(n // 8, dtype=torch.uint8), "dtype": torch.zeros(n // 8, dtype=torch.int8),
                "size": torch.zeros(n // 8 + 1, dtype=torch.uint8), "obj": NOT_A_TENSOR}[col[0]]
        return ops.mx_ste_backward(g, mask, col[1])
    return rows, cols, call


GRIDS = {
    "ops.mx_quantize_axis": lambda: _quantize_grid(ops.mx_quantize_axis, "return_mask", (False, True)),
    "llm_qat_amd.mx_quantize_axis": lambda: _quantize_grid(llm_qat_amd.mx_quantize_axis, "ste", ("identity", "clip", "mask")),
    "ops.mx_export": _export_grid,
    "ops.mx_ste_backward": _ste_grid,
}


def observe(name):
    """-> [[(exception type's name, message)]]: the grid of `name` as the imported package answers it"""
    rows, cols, call = GRIDS[name]()
    grid = []
    for row in rows:
        grid.append([])
        for col in cols:
            try:
                call(row, col)
                grid[-1].append(("none", ""))
            except Exception as e:  # noqa: BLE001 -- the table holds whatever is raised
                grid[-1].append((type(e).__name__, str(e)))
    return rows, cols, grid


_NO_CPU = ": tensor is on 'cpu'. llm_qat_amd runs on MI355X only and has no CPU fallback; move the tensor to the GPU (or use the reference implementation on CPU)."
MESSAGES = {
    "A": ("RuntimeError", "mx_quantize" + _NO_CPU),
    "B": ("ValueError", "mx_quantize: unknown scale_rule 'up': one of floor, ceil"),
    "C": ("ValueError", "MX formats need a last dimension that is a multiple of 32, got 48"),
    "D": ("ValueError", "mx_quantize: the column axis (axis=-2) does not serve rotate=True yet"),
    "E": ("ValueError", "mx_quantize: the column axis (axis=-2) does not serve return_mask=True yet"),
    "F": ("ValueError", "mx_quantize: axis=-2 needs a second-to-last dimension that is a multiple of 32, got 48"),
    "G": ("ValueError", "mx_quantize: axis=5: MX blocks run along the last axis (-1) or the one before it (-2)"),
    "H": ("ValueError", "unknown MX format 'mxfp5': one of mxfp4, mxfp6_e2m3, mxfp6_e3m2, mxfp8_e4m3, mxfp8_e5m2"),
    "I": ("TypeError", "mx_quantize: expected a torch.Tensor, got list"),
    "J": ("ValueError", "mx_quantize: unknown ste 'mask': one of identity, clip"),
    "K": ("ValueError", "mx_quantize: the column axis (axis=-2) does not serve ste=clip yet"),
    "L": ("RuntimeError", "mx_export" + _NO_CPU),
    "M": ("ValueError", "mx_export: unknown scale_rule 'up': one of floor, ceil"),
    "N": ("ValueError", "mx_export: the block-Hadamard rotation needs a last dimension that is a multiple of 64, got 32"),
    "O": ("ValueError", "'mxfp6_e2m3': FP6 formats have no export packing"),
    "P": ("TypeError", "mx_export: expected a torch.Tensor, got list"),
    "Q": ("RuntimeError", "mx_ste_backward" + _NO_CPU),
    "R": ("TypeError", "mx_ste_backward: the mask is a uint8 bitmap (mx_quantize(return_mask=True)), got torch.int8"),
    "S": ("ValueError", "mx_ste_backward: the mask holds 17 bytes, the gradient 128 elements: one bit per element is 16 bytes"),
    "T": ("TypeError", "mx_ste_backward: expected a torch.Tensor mask, got list"),
    "U": ("ValueError", "mx_ste_backward: the block-Hadamard rotation needs a last dimension that is a multiple of 64, got 32"),
    "V": ("ValueError", "mx_ste_backward: the mask holds 9 bytes, the gradient 64 elements: one bit per element is 8 bytes"),
    "W": ("ValueError", "mx_ste_backward: the gradient needs a last dimension that is a multiple of 32, got shape (2, 48)"),
    "X": ("TypeError", "mx_ste_backward: expected a torch.Tensor, got list"),
}
TABLE = {   # one string per row of the grid, one letter (MESSAGES) per column
    "ops.mx_quantize_axis": [     # columns: ceil x (no mask, mask) x (no rotate, rotate), then the same under the bad rule
        "AAAABBBB",   # cpu, mxfp4, axis -1, good shape
        "CCCCBBBB",   # cpu, mxfp4, axis -1, bad shape
        "ADEDBDED",   # cpu, mxfp4, axis -2, good shape
        "FDEDBDED",   # cpu, mxfp4, axis -2, bad shape
        "GGGGGGGG",   # cpu, mxfp4, axis 5
        "GGGGGGGG",
        "HHHHBBBB",   # cpu, mxfp5, axis -1, good shape
        "HHHHBBBB",   # cpu, mxfp5, axis -1, bad shape
        "HDEDBDED",   # cpu, mxfp5, axis -2, good shape
        "HDEDBDED",   # cpu, mxfp5, axis -2, bad shape
        "GGGGGGGG",   # cpu, mxfp5, axis 5
        "GGGGGGGG",
        "IIIIBBBB",   # not a tensor: mxfp4 at axis -1, -2, 5, then mxfp5
        "IIIIBBBB",
        "IIIIBBBB",
        "IIIIBBBB",
        "IIIIBBBB",
        "IIIIBBBB",
    ],
    "llm_qat_amd.mx_quantize_axis": [     # columns: ceil x (identity, clip, "mask") x (no rotate, rotate), then the same under the bad rule
        "AAAAJJBBBBBB",   # cpu, mxfp4, axis -1, good shape
        "CCCCCCCCCCCC",   # cpu, mxfp4, axis -1, bad shape
        "ADKDJJBBBBBB",   # cpu, mxfp4, axis -2, good shape
        "FFFFFFFFFFFF",   # cpu, mxfp4, axis -2, bad shape
        "GGGGGGGGGGGG",   # cpu, mxfp4, axis 5
        "GGGGGGGGGGGG",
        "HHHHHHHHHHHH",   # cpu, mxfp5, axes -1, -1, -2, -2
        "HHHHHHHHHHHH",
        "HHHHHHHHHHHH",
        "HHHHHHHHHHHH",
        "GGGGGGGGGGGG",   # cpu, mxfp5, axis 5
        "GGGGGGGGGGGG",
        "IIIIIIIIIIII",   # not a tensor
        "IIIIIIIIIIII",
        "IIIIIIIIIIII",
        "IIIIIIIIIIII",
        "IIIIIIIIIIII",
        "IIIIIIIIIIII",
    ],
    "ops.mx_export": [     # columns: ceil x (no rotate, rotate), then the bad rule
        "LLMM",   # cpu, mxfp4, (2, 64)
        "LNMM",   # cpu, mxfp4, (2, 32)
        "CCMM",   # cpu, mxfp4, (2, 48)
        "OOMM",   # cpu, mxfp6_e2m3, (2, 64)
        "OOMM",   # cpu, mxfp6_e2m3, (2, 32)
        "CCMM",   # cpu, mxfp6_e2m3, (2, 48)
        "HHMM",   # cpu, mxfp5
        "HHMM",
        "HHMM",
        "PPMM",   # not a tensor: mxfp4, mxfp6_e2m3, mxfp5
        "PPMM",
        "PPMM",
    ],
    "ops.mx_ste_backward": [     # columns: mask (good, int8, one byte too many, not a tensor) x (no rotate, rotate)
        "QQRRSSTT",   # gradient (2, 64)
        "QURUVUTT",   # gradient (2, 32)
        "WWWWWWTT",   # gradient (2, 48)
        "XXXXXXTT",   # not a tensor
    ],
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_every_cell_of_the_refusal_table_answers_as_before_the_helpers_were_folded(name):
    rows, cols, grid = observe(name)
    assert len(TABLE[name]) == len(rows) and all(len(line) == len(cols) for line in TABLE[name])
    wrong = [(row, col, got, MESSAGES[TABLE[name][i][j]]) for i, row in enumerate(rows) for j, col in enumerate(cols)
             for got in (grid[i][j],) if got != MESSAGES[TABLE[name][i][j]]]
    assert not wrong, f"{len(wrong)} cells differ, first (row, column, got, recorded): {wrong[:3]}"


def test_the_table_holds_every_single_fault_and_the_device_check_last():
    """what the grids are built to contain, read off the recorded table itself"""
    kinds = {MESSAGES[c][0] for lines in TABLE.values() for line in lines for c in line}
    assert kinds == {"ValueError", "TypeError", "RuntimeError"}          # never "none": no cell passes on the CPU
    for name in GRIDS:
        assert MESSAGES[TABLE[name][0][0]][0] == "RuntimeError" and "no CPU" in MESSAGES[TABLE[name][0][0]][1], name
    texts = " | ".join(m for _, m in MESSAGES.values())
    for part in ("unknown MX format", "axis=5", "last dimension that is a multiple of 32", "second-to-last dimension", "unknown scale_rule",
                 "unknown ste", "return_mask=True yet", "rotate=True yet", "ste=clip yet", "FP6 formats have no export packing",
                 "block-Hadamard rotation", "uint8 bitmap", "one bit per element", "expected a torch.Tensor"):
        assert part in texts, part


# ---- 2. the dispatch tables ------------------------------------------------------------------------------------------------------------------

QUANT_OPS = ("mx_fake_quant_op", "mx_fake_quant_rot_op", "mx_fake_quant_rule_op", "mx_fake_quant_clip_op", "mx_fake_quant_cols_op")
EXPORT_OPS = ("mx_export_op", "mx_export_rot_op", "mx_export_rule_op")


def _record_ops(monkeypatch, names):
    calls = []
    for name in names:
        def op(*args, _name=name, **kwargs):
            calls.append((_name, args, kwargs))
            return ("y", "mask") if _name == "mx_fake_quant_clip_op" else "y"
        monkeypatch.setattr(compiled, name, op)
    return calls


def test_mx_fake_quant_reaches_the_op_of_each_combination(monkeypatch):
    calls = _record_ops(monkeypatch, QUANT_OPS)
    x = object()
    for rotate in (False, True):
        for rule in ("floor", "ceil"):
            for clip in (False, True):
                if clip:
                    want = ("mx_fake_quant_clip_op", (x, "mxfp4", rotate, rule), {})
                elif rule != "floor":
                    want = ("mx_fake_quant_rule_op", (x, "mxfp4", rotate, rule), {})
                else:
                    want = ("mx_fake_quant_rot_op" if rotate else "mx_fake_quant_op", (x, "mxfp4"), {})
                for args in ((x, "mxfp4", rotate, rule, clip), (x, "mxfp4", rotate, rule, clip, -1)):     # axis defaults to the last one
                    del calls[:]
                    assert compiled.mx_fake_quant(*args) == "y"
                    assert calls == [want], (rotate, rule, clip)
                del calls[:]
                if rotate or clip:      # not served along the column axis (the public functions refuse them before they get here)
                    with pytest.raises(ValueError, match="column axis"):
                        compiled.mx_fake_quant(x, "mxfp4", rotate, rule, clip, -2)
                    assert calls == []
                else:
                    assert compiled.mx_fake_quant(x, "mxfp4", rotate, rule, clip, -2) == "y"
                    assert calls == [("mx_fake_quant_cols_op", (x, "mxfp4", rule), {})]


def test_mx_export_reaches_the_op_of_each_combination(monkeypatch):
    calls = _record_ops(monkeypatch, EXPORT_OPS)
    x = object()
    for rotate in (False, True):
        for rule in ("floor", "ceil"):
            del calls[:]
            assert compiled.mx_export(x, "mxfp8_e4m3", rotate, rule) == "y"
            if rule != "floor":
                assert calls == [("mx_export_rule_op", (x, "mxfp8_e4m3", rotate, rule), {})]
            else:
                assert calls == [("mx_export_rot_op" if rotate else "mx_export_op", (x, "mxfp8_e4m3"), {})]


@pytest.mark.parametrize("compiling", [False, True])
def test_mx_apply_carries_the_axis_to_either_side(monkeypatch, compiling):
    seen = {"compiled": [], "eager": []}
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: compiling)
    monkeypatch.setattr(compiled, "mx_fake_quant", lambda *a: seen["compiled"].append(a))
    monkeypatch.setattr(U._MXQuantizer, "apply", staticmethod(lambda *a: seen["eager"].append(a)))
    x = torch.zeros(64, 64, requires_grad=True)
    U._mx_apply(x, "mxfp4", True, "ceil", "clip")
    U._mx_apply(x, "mxfp4", False, "floor", "identity", -2)
    U._mx_apply(x.detach(), "mxfp4", False, "floor", "clip", -1)            # no gradient will come: no bitmap
    with torch.no_grad():
        U._mx_apply(x, "mxfp4", False, "floor", "clip", -1)
    got = seen["compiled" if compiling else "eager"]
    assert seen["eager" if compiling else "compiled"] == []
    assert [a[1:] for a in got] == [("mxfp4", True, "ceil", True, -1), ("mxfp4", False, "floor", False, -2),
                                    ("mxfp4", False, "floor", False, -1), ("mxfp4", False, "floor", False, -1)]
    assert got[0][0] is x and got[1][0] is x


def test_the_public_pair_validates_and_then_applies(monkeypatch):
    seen = []
    monkeypatch.setattr(mx_quant, "_mx_apply", lambda *a: seen.append(a))
    x = torch.zeros(2, 64, 64)
    llm_qat_amd.mx_quantize(x, "mxfp4", rotate=1, scale_rule="ceil", ste="clip")
    llm_qat_amd.mx_quantize_axis(x, "mxfp4")
    llm_qat_amd.mx_quantize_axis(x, "mxfp8_e4m3", scale_rule="ceil", axis=1)                  # the non-negative spelling of -2
    llm_qat_amd.mx_quantize_axis(x, "mxfp4", rotate=True, axis=2)
    assert [a[1:] for a in seen] == [("mxfp4", True, "ceil", "clip", -1), ("mxfp4", False, "floor", "identity", -1),
                                     ("mxfp8_e4m3", False, "ceil", "identity", -2), ("mxfp4", True, "floor", "identity", -1)]


def test_the_folded_names_are_gone_and_the_ops_stay():
    assert not hasattr(U, "_MXColsQuantizer") and not hasattr(ops, "_mx_quantize_cols")
    for name in ("mx_fake_quant", "mx_fake_quant_rot", "mx_fake_quant_rule", "mx_fake_quant_clip", "mx_fake_quant_cols", "mx_ste_backward",
                 "mx_block_rotate", "mx_export", "mx_export_rot", "mx_export_rule", "mx_matmul"):
        assert hasattr(torch.ops.llmqat_amd, name), name
    schema = lambda op: str(op._opoverload._schema)
    assert schema(compiled.mx_fake_quant_op) == "llmqat_amd::mx_fake_quant(Tensor x, str fmt) -> Tensor"
    assert schema(compiled.mx_fake_quant_rot_op) == "llmqat_amd::mx_fake_quant_rot(Tensor x, str fmt) -> Tensor"
    assert schema(compiled.mx_fake_quant_rule_op) == "llmqat_amd::mx_fake_quant_rule(Tensor x, str fmt, bool rotate, str scale_rule) -> Tensor"
    assert schema(compiled.mx_fake_quant_clip_op) == "llmqat_amd::mx_fake_quant_clip(Tensor x, str fmt, bool rotate, str scale_rule) -> (Tensor, Tensor)"
    assert schema(compiled.mx_export_op) == "llmqat_amd::mx_export(Tensor x, str fmt) -> (Tensor, Tensor)"
    assert schema(compiled.mx_export_rot_op) == "llmqat_amd::mx_export_rot(Tensor x, str fmt) -> (Tensor, Tensor)"
    assert schema(compiled.mx_export_rule_op) == "llmqat_amd::mx_export_rule(Tensor x, str fmt, bool rotate, str scale_rule) -> (Tensor, Tensor)"


# ---- 3. the fake implementations, on meta tensors ---------------------------------------------------------------------------------------------

def _meta(shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype, device="meta")


QUANT_CALLS = {   # op -> (its arguments after x for (rotate, rule), whether it serves that pair)
    "mx_fake_quant_op": lambda rotate, rule: ("mxfp4",) if (rotate, rule) == (False, "floor") else None,
    "mx_fake_quant_rot_op": lambda rotate, rule: ("mxfp4",) if (rotate, rule) == (True, "floor") else None,
    "mx_fake_quant_rule_op": lambda rotate, rule: ("mxfp4", rotate, rule),
    "mx_fake_quant_clip_op": lambda rotate, rule: ("mxfp4", rotate, rule),
    "mx_fake_quant_cols_op": lambda rotate, rule: None if rotate else ("mxfp4", rule),
}


@pytest.mark.parametrize("name", QUANT_OPS)
def test_quantizer_fakes_give_the_shapes_and_dtypes(name):
    op = getattr(compiled, name)
    for dtype in (torch.bfloat16, torch.float32):
        x = _meta((64, 3, 128), dtype).transpose(0, 1)                    # [3, 64, 128], not contiguous: the result is
        for rotate in (False, True):
            for rule in ("floor", "ceil"):
                args = QUANT_CALLS[name](rotate, rule)
                if args is None:
                    continue
                out = op(x, *args)
                y = out[0] if name == "mx_fake_quant_clip_op" else out
                assert y.shape == x.shape and y.dtype == dtype and y.is_contiguous() and y.device.type == "meta"
                if name == "mx_fake_quant_clip_op":
                    assert len(out) == 2 and out[1].shape == (3 * 64 * 128 // 8,) and out[1].dtype == torch.uint8
                else:
                    assert isinstance(out, torch.Tensor)


def test_quantizer_fakes_raise_the_messages():
    for name in QUANT_OPS:
        op, cols = getattr(compiled, name), name == "mx_fake_quant_cols_op"
        first = [a for a in (QUANT_CALLS[name](r, "floor") for r in (False, True)) if a is not None][0]
        with pytest.raises(ValueError, match="unknown MX format 'mxfp5': one of mxfp4, mxfp6_e2m3"):
            op(_meta((64, 64)), BAD_FMT, *first[1:])
        if cols:
            with pytest.raises(ValueError, match="mx_quantize: axis=-2 needs a second-to-last dimension that is a multiple of 32, got 48"):
                op(_meta((48, 64)), *first)
            with pytest.raises(ValueError, match="mx_quantize: axis=-2 needs a tensor with at least two dimensions, got 1"):
                op(_meta((64,)), *first)
            assert op(_meta((64, 3)), *first).shape == (64, 3)            # the last dimension is free there
        else:
            with pytest.raises(ValueError, match="MX formats need a last dimension that is a multiple of 32, got 48"):
                op(_meta((64, 48)), *first)
        if len(first) > 1:     # the op takes a rule
            with pytest.raises(ValueError, match="mx_quantize: unknown scale_rule 'up': one of floor, ceil"):
                op(_meta((64, 64)), *[BAD_RULE if a == "floor" else a for a in first])
    for name, args in (("mx_fake_quant_rot_op", ("mxfp4",)), ("mx_fake_quant_rule_op", ("mxfp4", True, "ceil")), ("mx_fake_quant_clip_op", ("mxfp4", True, "floor"))):
        with pytest.raises(ValueError, match="mx_quantize: the block-Hadamard rotation needs a last dimension that is a multiple of 64, got 96"):
            getattr(compiled, name)(_meta((2, 96)), *args)
    # two faults at once: the format answers before the rule, the rule before the rotation's width
    with pytest.raises(ValueError, match="unknown MX format"):
        compiled.mx_fake_quant_rule_op(_meta((2, 96)), BAD_FMT, True, BAD_RULE)
    with pytest.raises(ValueError, match="unknown scale_rule"):
        compiled.mx_fake_quant_clip_op(_meta((2, 96)), "mxfp4", True, BAD_RULE)


EXPORT_CALLS = {"mx_export_op": lambda fmt: (False, (fmt,)), "mx_export_rot_op": lambda fmt: (True, (fmt,)),
                "mx_export_rule_op": lambda fmt: (True, (fmt, True, "ceil"))}


@pytest.mark.parametrize("name", EXPORT_OPS)
def test_export_fakes_give_the_shapes_and_raise_the_messages(name):
    op = getattr(compiled, name)
    x = _meta((3, 2, 128))
    for fmt, ebytes in (("mxfp4", 64), ("mxfp8_e4m3", 128), ("mxfp8_e5m2", 128)):
        e, s = op(x, *EXPORT_CALLS[name](fmt)[1])
        assert e.shape == (3, 2, ebytes) and s.shape == (3, 2, 4) and e.dtype == s.dtype == torch.uint8
    rotates, args = EXPORT_CALLS[name]("mxfp4")
    with pytest.raises(ValueError, match="unknown MX format 'mxfp5'"):
        op(x, BAD_FMT, *args[1:])
    with pytest.raises(ValueError, match="MX formats need a last dimension that is a multiple of 32, got 48"):
        op(_meta((2, 48)), *args)
    with pytest.raises(ValueError, match="'mxfp6_e3m2': FP6 formats have no export packing"):
        op(x, "mxfp6_e3m2", *args[1:])
    if rotates:
        with pytest.raises(ValueError, match="mx_export: the block-Hadamard rotation needs a last dimension that is a multiple of 64, got 96"):
            op(_meta((2, 96)), *args)
        with pytest.raises(ValueError, match="block-Hadamard"):          # the rotation's width answers before the missing packing
            op(_meta((2, 96)), "mxfp6_e3m2", *args[1:])
    else:
        assert op(_meta((2, 96)), *args)[1].shape == (2, 3)
    if name == "mx_export_rule_op":
        with pytest.raises(ValueError, match="mx_export: unknown scale_rule 'up': one of floor, ceil"):
            op(_meta((2, 96)), "mxfp4", True, BAD_RULE)                   # ... and the rule before the rotation's width


def test_the_shared_fakes_called_directly():
    """one function per family stands behind the ops above"""
    x = _meta((64, 72), torch.float32)
    y, m = compiled._mx_quant_fake(_meta((2, 64)), "mxfp6_e2m3", True, "ceil", True)
    assert y.shape == (2, 64) and m.shape == (16,) and m.dtype == torch.uint8
    assert compiled._mx_quant_fake(x, "mxfp4", axis=-2).shape == (64, 72)
    with pytest.raises(ValueError, match="last dimension that is a multiple of 32, got 72"):
        compiled._mx_quant_fake(x, "mxfp4")
    e, s = compiled._mx_export_fake(_meta((5, 64)), "mxfp4", True, "ceil")
    assert e.shape == (5, 32) and s.shape == (5, 2)
