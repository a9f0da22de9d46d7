"""CPU tier of the fused SwiGLU: the fqa_ header and its binding, every refusal of the entry points in the order the
header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers below are never dereferenced), the recipe
against the eager chain bit for bit where ATen's CPU kernels allow it and against float64 everywhere, the CPU-tensor route against the
reference's own vectors (tests/golden/swiglu.npz), SwiGLUMLP, install(), convert(), the compiled ops' fake implementations and the Python
argument refusals."""
import ctypes
import os
import random
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import _lib, compiled, mlp, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import swiglu_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DY, G, U, Y, DG, DU = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000      # never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
DTYPE, SHAPE, NULL, LAUNCH, ARG, UNSUPPORTED = -1, -3, -4, -6, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 11008, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def fwd(*a):
    L = _lib.lib()
    rc = L.fqa_swiglu_fwd(*a, None)
    return rc, L.fq_last_error().decode()


def bwd(*a):
    L = _lib.lib()
    rc = L.fqa_swiglu_bwd(*a, None)
    return rc, L.fq_last_error().decode()


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_or_both_nan(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) and torch.equal(bits(a.nan_to_num(0.0)), bits(b.nan_to_num(0.0)))


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_act_header_names_equal_act_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_act.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqa_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.ACT_EXPORTS) == {"fqa_swiglu_fwd", "fqa_swiglu_bwd"}
    assert not re.findall(r"\bfq[tsilcn]?_[a-z0-9_]+\s*\(", src)     # nothing of the seven other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    others = (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS) | set(_lib.INFER_EXPORTS) | set(_lib.LOSS_EXPORTS)
              | set(_lib.CE_EXPORTS) | set(_lib.NORM_EXPORTS))
    assert not set(_lib.ACT_EXPORTS) & others
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.fqa_swiglu_fwd.argtypes == [vp, vp, vp, i64, i64, i64, i64, i32, vp] and L.fqa_swiglu_fwd.restype is i32
    assert L.fqa_swiglu_bwd.argtypes == [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, vp] and L.fqa_swiglu_bwd.restype is i32


def test_the_build_lists_the_new_unit_and_header():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_swiglu.hip", "fq_swiglu.h", "llmqat_fakequant_act.h"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

N3, N5 = (None,) * 3, (None,) * 5
FWD_REFUSALS = [
    # (gate, up, y, rows, cols, gate_stride, up_stride, dtype), code, part of the message
    (N3 + (-1, -1, -1, -1, 9), DTYPE, "unknown dtype"),
    (N3 + (-1, -1, -1, -1, -1), DTYPE, "unknown dtype"),
    (N3 + (-1, -1, -1, -1, F64), DTYPE, "float64"),
    (N3 + (-3, 8, 0, 0, BF16), SHAPE, "negative shape"),
    (N3 + (3, -8, 0, 0, F16), SHAPE, "negative shape"),
    (N3 + (0, 8, 0, 0, F32), SHAPE, "empty shape"),
    (N3 + (3, 0, -1, -1, BF16), SHAPE, "empty shape"),
    (N3 + (3, 8, 7, 8, BF16), SHAPE, "below cols"),
    (N3 + (3, 8, 8, 0, F32), SHAPE, "below cols"),
    (N3 + (3, 8, 16, -16, F16), SHAPE, "below cols"),
    (N3 + (2 ** 62, 2 ** 40, 2 ** 40, 2 ** 40, BF16), SHAPE, "rows * cols overflows"),
    (N3 + (2 ** 30, 8, 2 ** 60, 8, BF16), SHAPE, "stride + cols overflows"),
    (N3 + (2 ** 30, 8, 8, 2 ** 62, F32), SHAPE, "stride + cols overflows"),
    ((None, U, Y, 6, 8, 8, 8, BF16), NULL, "NULL"),
    ((G, None, Y, 6, 8, 8, 8, BF16), NULL, "NULL"),
    ((G, U, None, 6, 8, 8, 8, BF16), NULL, "NULL"),
    ((G, G, None, 2 ** 40, 4096, 4096, 4096, BF16), NULL, "NULL"),                       # the pointers come before the aliasing and the grid
    ((G, U, G, 6, 8, 8, 8, BF16), ARG, "in-place"),
    ((G, U, U, 6, 8, 16, 16, F32), ARG, "in-place"),
    ((G, U, G, 2 ** 40, 4096, 4096, 4096, F32), ARG, "in-place"),                         # the aliasing comes before the grid
    ((G, U, Y, 2 ** 33, 2048, 2048, 2048, BF16), UNSUPPORTED, "exceed one launch's grid"),       # the flat walk: 2^44 columns
    ((G, U, Y, 2 ** 33, 8, 16, 16, F32), UNSUPPORTED, "exceed one launch's grid"),               # the row-wise walk: a tile per row
]
BWD_REFUSALS = [
    # (dy, gate, up, dgate, dup, rows, cols, dy_stride, gate_stride, up_stride, dtype), code, part of the message
    (N5 + (-1, -1, -1, -1, -1, 9), DTYPE, "unknown dtype"),
    (N5 + (-1, -1, -1, -1, -1, F64), DTYPE, "float64"),
    (N5 + (-3, 8, 0, 0, 0, BF16), SHAPE, "negative shape"),
    (N5 + (0, 8, 0, 0, 0, F32), SHAPE, "empty shape"),
    (N5 + (3, 0, 0, 0, 0, F16), SHAPE, "empty shape"),
    (N5 + (3, 8, 7, 8, 8, BF16), SHAPE, "below cols"),
    (N5 + (3, 8, 8, 8, 7, BF16), SHAPE, "below cols"),
    (N5 + (2 ** 62, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40, BF16), SHAPE, "rows * cols overflows"),
    (N5 + (2 ** 30, 8, 2 ** 60, 8, 8, BF16), SHAPE, "stride + cols overflows"),
    ((None, G, U, DG, DU, 6, 8, 8, 8, 8, BF16), NULL, "dy / gate / up"),
    ((DY, None, U, DG, DU, 6, 8, 8, 8, 8, BF16), NULL, "dy / gate / up"),
    ((DY, G, None, DG, DU, 6, 8, 8, 8, 8, BF16), NULL, "dy / gate / up"),
    ((DY, G, U, None, None, 6, 8, 8, 8, 8, BF16), NULL, "both"),
    ((DY, G, DY, None, None, 2 ** 40, 4096, 4096, 4096, 4096, BF16), NULL, "both"),     # the pointers come before the aliasing and the grid
    ((DY, G, U, DY, DU, 6, 8, 8, 8, 8, BF16), ARG, "in-place (dgate"),
    ((DY, G, U, G, None, 6, 8, 8, 8, 8, F32), ARG, "in-place (dgate"),
    ((DY, G, U, U, DU, 6, 8, 8, 8, 8, F16), ARG, "in-place (dgate"),
    ((DY, G, U, DG, DY, 6, 8, 8, 8, 8, BF16), ARG, "in-place (dup"),
    ((DY, G, U, None, G, 6, 8, 8, 8, 8, BF16), ARG, "in-place (dup"),
    ((DY, G, U, DG, U, 6, 8, 8, 8, 8, BF16), ARG, "in-place (dup"),
    ((DY, G, U, DG, DG, 6, 8, 8, 8, 8, BF16), ARG, "same buffer"),
    ((DY, G, U, DG, DG, 2 ** 40, 4096, 4096, 4096, 4096, BF16), ARG, "same buffer"),    # the aliasing comes before the grid
    ((DY, G, U, DG, DU, 2 ** 33, 2048, 2048, 2048, 2048, BF16), UNSUPPORTED, "exceed one launch's grid"),
    ((DY, G, U, None, DU, 2 ** 33, 8, 16, 8, 8, F32), UNSUPPORTED, "exceed one launch's grid"),
]


@pytest.mark.parametrize("args, code, text", FWD_REFUSALS)
def test_every_forward_refusal_comes_back_with_its_code_in_the_stated_order(args, code, text):
    rc, msg = fwd(*args)
    assert rc == code, (rc, msg)
    assert text in msg, msg


@pytest.mark.parametrize("args, code, text", BWD_REFUSALS)
def test_every_backward_refusal_comes_back_with_its_code_in_the_stated_order(args, code, text):
    rc, msg = bwd(*args)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_every_served_dtype_passes_the_first_checks_and_a_single_row_ignores_its_strides():
    for dt in (F32, BF16, F16):
        assert fwd(*N3, 6, 11008, 11008, 22016, dt)[0] == NULL and bwd(*N5, 6, 11008, 11008, 22016, 22016, dt)[0] == NULL
        assert fwd(*N3, 1, 8, 2 ** 62, 8, dt)[0] == NULL       # (rows - 1) * stride is 0 whatever the stride


def test_fuzz_never_reaches_a_launch():
    rng = random.Random(27)
    L = _lib.lib()
    clamp = lambda v: max(-(2 ** 31), min(2 ** 31 - 1, v))      # noqa: E731
    most = (2 ** 63 - 1) // 4

    def bad_shape(rows, cols, strides):
        if rows <= 0 or cols <= 0 or rows * cols > most:
            return True
        return any(s < cols or (rows > 1 and (rows - 1) * s + cols > most) for s in strides)
    seen = set()
    for _ in range(400):                                   # hostile everything
        rows, cols, s0, s1, s2 = (rng.choice(INTS) for _ in range(5))
        rc = L.fqa_swiglu_fwd(*N3, rows, cols, s0, s1, clamp(rng.choice(INTS)), None)
        assert rc in (DTYPE, SHAPE, NULL), (rc, rows, cols)
        rc2 = L.fqa_swiglu_bwd(*N5, rows, cols, s0, s1, s2, clamp(rng.choice(INTS)), None)
        assert rc2 in (DTYPE, SHAPE, NULL), (rc2, rows, cols)
        assert L.fq_last_error() != b""
        seen |= {rc, rc2}
    for _ in range(400):       # the same hostile sizes behind a served dtype, so that the shape checks are the ones that answer
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        s0, s1, s2 = (rng.choice(INTS + [cols, cols, cols + 8]) for _ in range(3))
        dt = rng.choice((F32, BF16, F16))
        rc = L.fqa_swiglu_fwd(*N3, rows, cols, s0, s1, dt, None)
        assert rc == (SHAPE if bad_shape(rows, cols, (s0, s1)) else NULL), (rc, rows, cols, s0, s1)
        rc2 = L.fqa_swiglu_bwd(*N5, rows, cols, s0, s1, s2, dt, None)
        assert rc2 == (SHAPE if bad_shape(rows, cols, (s0, s1, s2)) else NULL), (rc2, rows, cols, s0, s1, s2)
        seen |= {rc, rc2}
    assert seen == {DTYPE, SHAPE, NULL}               # never 0, never FQ_ERR_LAUNCH: NULL pointers are never launchable


# ---- the recipe, the chain and float64 ------------------------------------------------------------------------------------------------------------

def wide_inputs(dtype, shape=(64, 11008), seed=1):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.randn(shape, generator=gen) * 3).to(dtype), torch.randn(shape, generator=gen).to(dtype), torch.randn(shape, generator=gen).to(dtype))


def test_the_recipe_equals_the_chain_bit_for_bit_where_atens_cpu_kernels_take_the_same_route():
    """bf16: y, dg, du.  fp16: y and du (ATen's CPU fp16 silu_backward takes another route: a few dozen of 704512 dg differ).  fp32 differs
    through the CPU's vectorised exp.  What is not compared here is held to the float64 caps below."""
    g, u, dy = wide_inputs(torch.bfloat16)
    y, dg, du = R.chain(g, u, dy)
    rdg, rdu = R.recipe_bwd(dy, g, u)
    assert torch.equal(bits(R.recipe_fwd(g, u)), bits(y)) and torch.equal(bits(rdg), bits(dg)) and torch.equal(bits(rdu), bits(du))
    g, u, dy = wide_inputs(torch.float16)
    y, dg, du = R.chain(g, u, dy)
    rdg, rdu = R.recipe_bwd(dy, g, u)
    assert torch.equal(bits(R.recipe_fwd(g, u)), bits(y)) and torch.equal(bits(rdu), bits(du))
    differ = int((rdg != dg).sum())
    print(f"fp16 dg: {differ} of {dg.numel()} elements differ from ATen's CPU silu_backward")
    assert differ < dg.numel() // 1000


def test_recipe_chain_and_cpu_route_stay_within_the_float64_caps():
    from llm_qat_amd import cpu_tensors
    was = cpu_tensors.ENABLED
    worst = [0.0, 0.0, 0.0]
    try:
        llm_qat_amd.allow_cpu_tensors(True)
        for name, (g, u, dy) in R.CASES().items():
            for dtype in DTYPES:
                gd, ud, dd = g.to(dtype), u.to(dtype), dy.to(dtype)
                ref = R.ref64(gd, ud, dd)
                gr, ur = gd.clone().requires_grad_(True), ud.clone().requires_grad_(True)
                yr = mlp.swiglu(gr, ur)
                route = (yr.detach(),) + torch.autograd.grad(yr, (gr, ur), dd)
                rdg, rdu = R.recipe_bwd(dd, gd, ud)
                for what, (y, dg, du) in (("recipe", (R.recipe_fwd(gd, ud), rdg, rdu)), ("chain", R.chain(gd, ud, dd)), ("route", route)):
                    m = R.measures(y, dg, du, gd, ud, dd, ref)
                    worst = [max(a, b) for a, b in zip(worst, m)]
                    assert m[0] <= R.Y_CAP and m[1] <= R.DG_CAP and m[2] <= R.DU_CAP, (name, dtype, what, m)
    finally:
        llm_qat_amd.allow_cpu_tensors(was)
    print("largest C_y, C_dg, C_du:", worst)


def test_the_caps_are_twice_the_eager_fp32_chains_measures():
    assert (R.Y_CAP, R.DG_CAP, R.DU_CAP) == (2 * R.EAGER_C_Y, 2 * R.EAGER_C_DG, 2 * R.EAGER_C_DU)
    m = R.eager_measures("cpu")
    assert set(m) == set(R.CASES()) and len(m) == 5
    for g, u, dy in R.CASES().values():
        assert torch.equal(g, g.bfloat16().float()) and torch.equal(u, u.bfloat16().float()) and torch.equal(dy, dy.bfloat16().float())
    worst = [max(v[i] for v in m.values()) for i in range(3)]
    print({k: tuple(round(t, 4) for t in v) for k, v in m.items()})
    for got, eager in zip(worst, (R.EAGER_C_Y, R.EAGER_C_DG, R.EAGER_C_DU)):
        assert 0.9 * eager <= got <= eager, (worst, eager)           # written down from the chain, rounded up in the second decimal


def test_the_measures_see_an_error_of_their_size():
    g, u, dy = R.CASES()["randn_s3"]
    ref = R.ref64(g, u, dy)
    y64, dg64, du64, _ = ref
    assert R.measures(y64, dg64, du64, g, u, dy, ref) == (0.0, 0.0, 0.0)
    for i, cap in enumerate((R.Y_CAP, R.DG_CAP, R.DU_CAP)):
        wrong = [y64.clone(), dg64.clone(), du64.clone()]
        wrong[i][1, 7] *= 1 + 2.0 ** -12          # one element, 4096 fp32 ulp off
        assert R.measures(*(t.float() for t in wrong), g, u, dy, ref)[i] > cap
    near = (g + 1.28).abs().argmin()              # where dg's factor crosses zero the measure stays finite and small for the fp32 chain
    y, dg, du = R.chain(g, u, dy)
    assert abs(float(g.reshape(-1)[near]) + 1.28) < 0.01 and R.measures(y, dg, du, g, u, dy, ref)[1] <= R.DG_CAP / 2
    h = (y64.half(), dg64.half(), du64.half())    # the output rounding is allowed for ...
    assert R.measures(*h, g.half(), u.half(), dy.half(), ref) == (0.0, 0.0, 0.0)
    assert R.measures(y64.half().float(), dg64.float(), du64.float(), g, u, dy, ref)[0] > R.Y_CAP      # ... only where the dtype has it


# ---- the reference's own vectors and the CPU-tensor route ---------------------------------------------------------------------------------------

def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "swiglu.npz"))

    def load(key, dtype):
        a = z[key]
        t = torch.from_numpy(a.view(np.int16).copy()).view(dtype) if a.dtype == np.uint16 else torch.from_numpy(a.copy())
        assert t.dtype is dtype, (key, t.dtype)
        return t
    for name in z["dtypes"]:
        for case in [f"c{c}" for c in z["cols"]] + ["special"]:
            k = f"{name}_{case}_"
            yield (str(name), case) + tuple(load(k + t, DT[str(name)]) for t in ("g", "u", "dy", "y", "dg", "du"))


def test_the_fixture_holds_the_three_dtypes_the_three_widths_and_the_special_row():
    cases = list(golden())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "swiglu.npz")) < 40 * 1024
    assert {c[0] for c in cases} == {"bf16", "f16", "f32"} and {c[1] for c in cases} == {"c7", "c33", "c256", "special"}
    inf, nan = float("inf"), float("nan")
    for name, case, g, u, dy, y, dg, du in cases:
        assert g.shape == u.shape == dy.shape == y.shape == dg.shape == du.shape and g.dim() == 2
        if case != "special":
            assert g.shape[1] == int(case[1:]) and all(torch.isfinite(t).all() for t in (y, dg, du))
            continue
        assert g.shape == (1, 40)
        gates, ups = g[0, ::4].float().tolist(), u[0, :4].float().tolist()
        assert gates[:2] == [inf, -inf] and gates[2] != gates[2] and gates[3:] == [-200.0, -104.0, -88.0, 88.0, 200.0, 0.0, -0.0]
        assert ups == [0.0, 1.0, -1.0, inf] and str(gates[-1]) == "-0.0"
        yy = y[0].float()
        assert yy[0:1].isnan().all()                                  # silu(+inf) * 0
        assert yy[4:8].isnan().all() and yy[8:12].isnan().all()       # silu(-inf) and a NaN gate: every up
        for k in (3, 4):                                              # g = -200, -104: exp(-g) overflows, silu = -0
            assert [str(v) for v in yy[4 * k:4 * k + 3].tolist()] == ["-0.0", "-0.0", "0.0"] and bool(yy[4 * k + 3].isnan())
        assert yy[4 * 7 + 1] == 200.0 and yy[4 * 8 + 1] == 0.0 and bool(yy[4 * 8 + 3].isnan())


def test_cpu_tensors_are_refused_by_default_and_served_bit_for_bit_after_the_opt_in():
    from llm_qat_amd import cpu_tensors
    was = cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(False)
        g, u, _ = R.CASES()["randn_s1"]
        lin = torch.nn.Linear(515, 515, bias=False)
        for f in (lambda: mlp.swiglu(g, u), lambda: mlp.SwiGLUMLP(lin, lin, lin)(g)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f()
        llm_qat_amd.allow_cpu_tensors(True)
        before = dict(ops.act_counts)
        for name, case, g, u, dy, y, dg, du in golden():
            gr, ur = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
            got = mlp.swiglu(gr, ur)
            assert got.dtype is y.dtype and same_or_both_nan(got, y), (name, case)
            gg, gu = torch.autograd.grad(got, (gr, ur), dy)
            assert same_or_both_nan(gg, dg) and same_or_both_nan(gu, du), (name, case)
        assert ops.act_counts == before                      # no launch, no copy: torch ops
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


# ---- SwiGLUMLP, install(), convert(), the package surface -----------------------------------------------------------------------------------------

class StockMLP(torch.nn.Module):
    """the shape of LlamaMLP (the reference's and Hugging Face's): three projections and act_fn"""

    def __init__(self, hidden=16, inter=24, act=None):
        super().__init__()
        self.gate_proj = QuantizeLinear(hidden, inter, bias=False, w_bits=4, a_bits=8)
        self.down_proj = QuantizeLinear(inter, hidden, bias=False, w_bits=4, a_bits=8)
        self.up_proj = QuantizeLinear(hidden, inter, bias=False, w_bits=4, a_bits=8)
        self.act_fn = act if act is not None else torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class SiLUActivation:        # Hugging Face's activation object, by its class name
    def __call__(self, x):
        return F.silu(x)


def test_the_module_holds_the_given_children_under_llamamlps_names():
    stock = StockMLP()
    m = mlp.SwiGLUMLP(stock.gate_proj, stock.up_proj, stock.down_proj)
    assert m.gate_proj is stock.gate_proj and m.up_proj is stock.up_proj and m.down_proj is stock.down_proj
    assert set(m.state_dict()) == set(stock.state_dict()) == {"gate_proj.weight", "up_proj.weight", "down_proj.weight"}
    assert StockMLP().load_state_dict(m.state_dict()).missing_keys == [] and m.load_state_dict(stock.state_dict()).unexpected_keys == []
    assert [n for n, _ in m.named_children()] == ["gate_proj", "up_proj", "down_proj"]


def test_install_subclasses_the_modules_class_returns_the_old_one_and_can_be_undone():
    from llm_qat_amd import cpu_tensors
    ns = types.ModuleType("modeling_stand_in")
    ns.LlamaMLP = StockMLP
    assert mlp.install(ns) is StockMLP and ns.LlamaMLP is not StockMLP and issubclass(ns.LlamaMLP, StockMLP)
    assert ns.LlamaMLP.__name__ == "StockMLP" and ns.LlamaMLP.__init__ is StockMLP.__init__
    built = ns.LlamaMLP(16, 24)
    assert isinstance(built, StockMLP) and set(built.state_dict()) == set(StockMLP().state_dict())
    x = torch.randn(2, 3, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):        # the fused forward is the one that runs: CPU tensors are refused
        built(x)
    gelu = ns.LlamaMLP(16, 24, torch.nn.GELU())
    was = cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(True)
        assert torch.equal(gelu(x), StockMLP.forward(gelu, x))        # another activation: the parent's forward
        assert torch.equal(built(x), StockMLP.forward(built, x))      # the CPU route is the chain
    finally:
        llm_qat_amd.allow_cpu_tensors(was)
    ns.LlamaMLP = StockMLP                                        # the undo
    assert mlp.install(ns) is StockMLP
    for wrong in (object(), {"LlamaMLP": 1}, StockMLP):
        with pytest.raises(TypeError, match="module object"):
            mlp.install(wrong)


def test_convert_swaps_the_silu_mlps_in_place_and_leaves_everything_else_alone():
    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mlp = StockMLP()
            self.functional = StockMLP(act=F.silu)
            self.hf = StockMLP(act=SiLUActivation())
            self.gelu = StockMLP(act=torch.nn.GELU())
            self.head = torch.nn.Linear(16, 4)
            self.layers = torch.nn.ModuleList([StockMLP(), mlp.SwiGLUMLP(torch.nn.Linear(16, 24), torch.nn.Linear(16, 24), torch.nn.Linear(24, 16))])
    model = Block().eval()
    params = dict(model.named_parameters())
    children = {n: (m.gate_proj, m.up_proj, m.down_proj) for n, m in (("mlp", model.mlp), ("functional", model.functional), ("hf", model.hf))}
    kept = (model.gelu, model.head, model.layers[1])
    keys = list(model.state_dict())
    assert mlp.convert(model) == 4
    for n, trio in children.items():
        m = getattr(model, n)
        assert type(m) is mlp.SwiGLUMLP and (m.gate_proj, m.up_proj, m.down_proj) == trio and not m.training
    assert type(model.layers[0]) is mlp.SwiGLUMLP and (model.gelu, model.head, model.layers[1]) == kept and type(model.gelu) is StockMLP
    after = dict(model.named_parameters())
    assert set(after) == set(params) and all(after[k] is params[k] for k in params)       # the Parameter objects are kept
    assert set(model.state_dict()) == set(keys)
    assert mlp.convert(model) == 0
    with pytest.raises(TypeError, match="torch.nn.Module"):
        mlp.convert([model])


def test_the_public_names_live_in_the_submodule():
    assert llm_qat_amd.mlp is mlp and mlp.__all__ == ["swiglu", "SwiGLUMLP", "install", "convert"]
    for name in ["mlp"] + mlp.__all__:
        assert name not in llm_qat_amd.__all__, name
    assert not hasattr(llm_qat_amd, "swiglu") and not hasattr(llm_qat_amd, "SwiGLUMLP")
    assert llm_qat_amd.__all__[-2:] == ["MXLinear", "convert_to_mx_inference"] and len(llm_qat_amd.__all__) == len(set(llm_qat_amd.__all__))
    assert set(ops.act_counts) == {"fwd_launch", "bwd_launch", "copy_route"}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "llm_qat_amd.mlp" in text and "mlp.install(" in text and "mlp.convert(" in text


# ---- the compiled ops' fake implementations ----------------------------------------------------------------------------------------------------

def test_fake_ops_shapes_and_dtypes_on_meta_tensors():
    assert str(compiled.swiglu_fwd_op._opoverload._schema) == "llmqat_amd::swiglu_fwd(Tensor gate, Tensor up) -> Tensor"
    assert str(compiled.swiglu_bwd_op._opoverload._schema) == \
        "llmqat_amd::swiglu_bwd(Tensor dy, Tensor gate, Tensor up, bool need_dgate, bool need_dup) -> (Tensor, Tensor)"
    for dtype in DTYPES:
        for shape in ((6, 515), (2, 3, 4096), (33,)):
            g, u = torch.empty(shape, dtype=dtype, device="meta"), torch.empty(shape, dtype=dtype, device="meta")
            y = torch.ops.llmqat_amd.swiglu_fwd(g, u)
            assert y.device.type == "meta" and tuple(y.shape) == shape and y.dtype is dtype and y.is_contiguous()
            dg, du = torch.ops.llmqat_amd.swiglu_bwd(y, g, u, True, True)
            assert tuple(dg.shape) == tuple(du.shape) == shape and dg.dtype is du.dtype is dtype
            dg, du = torch.ops.llmqat_amd.swiglu_bwd(y, g, u, True, False)
            assert tuple(dg.shape) == shape and du.numel() == 0
            dg, du = torch.ops.llmqat_amd.swiglu_bwd(y, g, u, False, True)
            assert dg.numel() == 0 and tuple(du.shape) == shape
    halves = torch.empty(4, 16, dtype=torch.bfloat16, device="meta").chunk(2, -1)
    assert torch.ops.llmqat_amd.swiglu_fwd(*halves).is_contiguous()
    g = torch.empty(4, 8, dtype=torch.float64, device="meta")
    with pytest.raises(TypeError, match="not served"):
        torch.ops.llmqat_amd.swiglu_fwd(g, g)
    with pytest.raises(ValueError, match="shape mismatch"):
        torch.ops.llmqat_amd.swiglu_fwd(g.float(), torch.empty(4, 9, device="meta"))


# ---- Python argument refusals (all before any launch; the device check is the last of them, so CPU tensors reach the others) -----------------

def test_python_argument_refusals():
    g, u = torch.zeros(2, 3, 8), torch.ones(2, 3, 8)
    before = dict(ops.act_counts)
    for f in (mlp.swiglu, ops.swiglu_forward, lambda a, b: ops.swiglu_backward(a, a, b)):
        with pytest.raises(TypeError, match="float64 is not served"):
            f(g.double(), u.double())
        with pytest.raises(TypeError, match="torch.int32 is not served"):
            f(g.int(), u.int())
        with pytest.raises(TypeError, match="no promotion"):
            f(g.bfloat16(), u)
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(g, None)
        with pytest.raises(ValueError, match="no broadcasting"):
            f(g, u[:, :1])
        with pytest.raises(ValueError, match="no broadcasting"):
            f(g, u[0])
        with pytest.raises(ValueError, match="at least one dimension"):
            f(torch.zeros(()), torch.zeros(()))
        with pytest.raises(ValueError, match="gate is on cpu, up on meta"):
            f(g, u.to("meta"))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.swiglu_forward(g, u)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.swiglu_backward(g, g, u)
    with pytest.raises(ValueError, match="neither dgate nor dup"):
        ops.swiglu_backward(g, g, u, False, False)
    with pytest.raises(ValueError, match="dy is the gradient of y"):
        ops.swiglu_backward(g[0], g, u)
    assert ops.act_counts == before
