"""CPU tier of the fused RMSNorm: the fqn_ header and its binding, every refusal of the entry points in the order the
header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers below are never dereferenced), the recipe
against the reference's chain bit for bit, the contract's backward against float64 autograd, the CPU-tensor route against the reference's
own vectors (tests/golden/rms_norm.npz), the RMSNorm class, install(), convert(), the compiled ops' fake implementations and the Python
argument refusals."""
import ctypes
import math
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, compiled, norm, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import rms_norm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, W, Y, RS, G, DX, DW, WS = 0x1000, 0x2000, 0x3000, 0x4004, 0x5000, 0x6000, 0x7000, 0x8000      # never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
DTYPE, SHAPE, NULL, WORKSPACE, LAUNCH, ARG, UNSUPPORTED = -1, -3, -4, -5, -6, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 11008, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]
FLOATS = [0.0, 1e-6, 1e-5, 1.0, 3e38, -0.0, -1e-6, -1.0, float("nan"), float("inf"), float("-inf")]
SERVED = [(F32, F32), (BF16, BF16), (F16, F16), (F32, BF16), (F32, F16), (BF16, F32), (F16, F32)]
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def fwd(*a):
    L = _lib.lib()
    rc = L.fqn_rms_norm_fwd(*a, None)
    return rc, L.fq_last_error().decode()


def bwd(*a):
    L = _lib.lib()
    rc = L.fqn_rms_norm_bwd(*a, None)
    return rc, L.fq_last_error().decode()


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_norm_header_names_equal_norm_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_norm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqn_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.NORM_EXPORTS) == {"fqn_rms_norm_fwd", "fqn_rms_norm_bwd", "fqn_rms_norm_bwd_parts", "fqn_rms_norm_bwd_workspace_bytes"}
    assert not re.findall(r"\bfq[tsilc]?_[a-z0-9_]+\s*\(", src)      # nothing of the six other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    others = (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS) | set(_lib.INFER_EXPORTS) | set(_lib.LOSS_EXPORTS)
              | set(_lib.CE_EXPORTS))
    assert not set(_lib.NORM_EXPORTS) & others
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32, f32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert L.fqn_rms_norm_fwd.argtypes == [vp, vp, vp, vp, i64, i64, f32, i32, i32, vp] and L.fqn_rms_norm_fwd.restype is i32
    assert L.fqn_rms_norm_bwd.argtypes == [vp, vp, vp, vp, vp, vp, vp, sz, i64, i64, i32, i32, vp] and L.fqn_rms_norm_bwd.restype is i32
    assert L.fqn_rms_norm_bwd_parts.argtypes == [i64, i64] and L.fqn_rms_norm_bwd_parts.restype is i64
    assert L.fqn_rms_norm_bwd_workspace_bytes.argtypes == [i64, i64] and L.fqn_rms_norm_bwd_workspace_bytes.restype is sz


def test_the_build_lists_the_new_unit_and_header():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_rms_norm.hip", "fq_rms_norm.h", "fq_rows.h", "llmqat_fakequant_norm.h"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

N4, N7 = (None,) * 4, (None,) * 7
NAN, INF = float("nan"), float("inf")
FWD_REFUSALS = [
    # (x, w, y, rstd, rows, cols, eps, x_dtype, w_dtype), code, part of the message
    (N4 + (-1, -1, -1.0, 9, BF16), DTYPE, "unknown dtype"),
    (N4 + (-1, -1, -1.0, BF16, -1), DTYPE, "unknown dtype"),
    (N4 + (-1, -1, -1.0, F64, BF16), DTYPE, "float64"),
    (N4 + (-1, -1, -1.0, F32, F64), DTYPE, "float64"),
    (N4 + (-1, -1, -1.0, BF16, F16), DTYPE, "pair"),
    (N4 + (-1, -1, -1.0, F16, BF16), DTYPE, "pair"),
    (N4 + (-3, 8, -1.0, BF16, BF16), SHAPE, "negative shape"),
    (N4 + (3, -8, -1.0, F16, F32), SHAPE, "negative shape"),
    (N4 + (0, 8, -1.0, F32, F32), SHAPE, "empty shape"),
    (N4 + (3, 0, -1.0, BF16, F32), SHAPE, "empty shape"),
    (N4 + (2 ** 62, 2 ** 40, -1.0, BF16, BF16), SHAPE, "overflows"),
    (N4 + (6, 8, -1e-6, BF16, BF16), ARG, "eps"),
    (N4 + (6, 8, NAN, F32, BF16), ARG, "eps"),
    (N4 + (6, 8, INF, F16, F16), ARG, "eps"),
    (N4 + (6, 8, -INF, F16, F16), ARG, "eps"),
    ((None, W, Y, RS, 6, 8, 1e-6, BF16, BF16), NULL, "NULL"),
    ((X, None, Y, RS, 6, 8, 1e-6, BF16, BF16), NULL, "NULL"),
    ((X, W, None, RS, 6, 8, 0.0, BF16, BF16), NULL, "NULL"),
    ((X, W, None, None, 2 ** 40, 4096, 0.0, BF16, BF16), NULL, "NULL"),                       # the pointers come before the aliasing and the grid
    ((X, W, X, RS, 6, 8, 1e-6, BF16, BF16), ARG, "in-place"),
    ((X, W, W, RS, 6, 8, 1e-6, F32, F32), ARG, "in-place"),
    ((X, W, X, None, 2 ** 40, 4096, 1e-6, F32, F32), ARG, "in-place"),                        # the aliasing comes before the grid
    ((X, W, Y, None, 2 ** 33, 2048, 1e-6, BF16, BF16), UNSUPPORTED, "exceed one launch's grid"),      # rstd may be NULL
    ((X, W, Y, RS, 2 ** 34, 8, 0.0, F32, BF16), UNSUPPORTED, "exceed one launch's grid"),
]
BWD_REFUSALS = [
    # (g, x, w, rstd, dx, dw, workspace, workspace_bytes, rows, cols, x_dtype, w_dtype), code, part of the message
    (N7 + (0, -1, -1, 9, BF16), DTYPE, "unknown dtype"),
    (N7 + (0, -1, -1, BF16, F64), DTYPE, "float64"),
    (N7 + (0, -1, -1, F16, BF16), DTYPE, "pair"),
    (N7 + (0, -3, 8, BF16, BF16), SHAPE, "negative shape"),
    (N7 + (0, 0, 8, F32, F32), SHAPE, "empty shape"),
    (N7 + (0, 3, 0, F16, F32), SHAPE, "empty shape"),
    (N7 + (0, 2 ** 62, 2 ** 40, BF16, BF16), SHAPE, "overflows"),
    ((None, X, W, RS, DX, DW, WS, 0, 6, 8, BF16, BF16), NULL, "g / x / w / rstd"),
    ((G, None, W, RS, DX, DW, WS, 0, 6, 8, BF16, BF16), NULL, "g / x / w / rstd"),
    ((G, X, None, RS, DX, DW, WS, 0, 6, 8, BF16, BF16), NULL, "g / x / w / rstd"),
    ((G, X, W, None, DX, DW, WS, 0, 6, 8, BF16, BF16), NULL, "g / x / w / rstd"),
    ((G, X, W, RS, None, None, WS, 0, 6, 8, BF16, BF16), NULL, "both"),
    ((G, X, W, RS, G, DW, None, 0, 6, 8, BF16, BF16), NULL, "workspace"),                     # the pointers come before the aliasing
    ((G, X, W, RS, G, DW, WS, 0, 6, 8, BF16, BF16), ARG, "in-place (dx"),
    ((G, X, W, RS, X, None, None, 0, 6, 8, BF16, BF16), ARG, "in-place (dx"),               # no dw: no workspace wanted
    ((G, X, W, RS, W, DW, WS, 0, 6, 8, F32, F32), ARG, "in-place (dx"),
    ((G, X, W, RS, DX, W, WS, 0, 6, 8, F32, F32), ARG, "in-place (dw"),
    ((G, X, W, RS, None, G, WS, 0, 6, 8, F32, F32), ARG, "in-place (dw"),                    # the aliasing comes before the workspace's size
    ((G, X, W, RS, DX, DW, WS, 6 * 8 * 4 - 1, 6, 8, BF16, BF16), WORKSPACE, "workspace too small"),
    ((G, X, W, RS, None, DW, WS, 0, 2 ** 20, 4096, BF16, F32), WORKSPACE, "workspace too small"),
    ((G, X, W, RS, DX, DW, WS, 2 ** 62, 1, 2 ** 36, BF16, BF16), UNSUPPORTED, "columns exceed one launch's grid"),
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


def test_every_served_pair_passes_the_first_checks_and_no_other_does():
    for xd in (F32, BF16, F16):
        for wd in (F32, BF16, F16):
            want = NULL if (xd, wd) in SERVED else DTYPE
            assert fwd(*N4, 6, 11008, 1e-6, xd, wd)[0] == want and bwd(*N7, 0, 6, 11008, xd, wd)[0] == want
    assert len(SERVED) == 7
    assert fwd(*N4, 6, 8, 0.0, BF16, BF16)[0] == NULL                 # eps = 0 is served


def test_the_chunks_of_the_backward_are_a_function_of_the_shape():
    L = _lib.lib()
    assert L.fqn_rms_norm_bwd_parts(2048, 4096) == 512 and L.fqn_rms_norm_bwd_workspace_bytes(2048, 4096) == 512 * 4096 * 4
    most = L.fqn_rms_norm_bwd_parts(10 ** 9, 64)
    assert most == 2048 and L.fqn_rms_norm_bwd_parts(10 ** 9, 2048) == 512 == L.fqn_rms_norm_bwd_parts(10 ** 9, 10 ** 9)
    assert L.fqn_rms_norm_bwd_parts(most, 64) == most and L.fqn_rms_norm_bwd_parts(3 * most - 1, 64) == most
    assert L.fqn_rms_norm_bwd_parts(most + 1, 64) == (most + 2) // 2
    for rows, cols in ((1, 1), (3, 7), (513, 4096), (1030, 64), (2049, 33), (4097, 2047), (10 ** 6, 5120)):
        parts = L.fqn_rms_norm_bwd_parts(rows, cols)
        rpp = -(-rows // parts)
        assert 1 <= parts <= min(rows, 512 if cols >= 2048 else 2048) and (parts - 1) * rpp < rows <= parts * rpp, (rows, cols, parts)
        assert L.fqn_rms_norm_bwd_workspace_bytes(rows, cols) == parts * cols * 4
    for rows, cols in ((0, 8), (8, 0), (-1, 8), (8, -1), (2 ** 62, 2 ** 40)):
        assert L.fqn_rms_norm_bwd_parts(rows, cols) == 0 and L.fqn_rms_norm_bwd_workspace_bytes(rows, cols) == 0


def test_fuzz_never_reaches_a_launch():
    rng = random.Random(25)
    L = _lib.lib()
    clamp = lambda v: max(-(2 ** 31), min(2 ** 31 - 1, v))      # noqa: E731
    bad_shape = lambda rows, cols: rows <= 0 or cols <= 0 or rows * cols > (2 ** 63 - 1) // 4      # noqa: E731
    seen = set()
    for _ in range(400):                                   # hostile everything
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        rc = L.fqn_rms_norm_fwd(*N4, rows, cols, rng.choice(FLOATS), clamp(rng.choice(INTS)), clamp(rng.choice(INTS)), None)
        assert rc in (DTYPE, SHAPE, ARG, NULL), (rc, rows, cols)
        rc2 = L.fqn_rms_norm_bwd(*N7, rng.choice(INTS) % 2 ** 64, rows, cols, clamp(rng.choice(INTS)), clamp(rng.choice(INTS)), None)
        assert rc2 in (DTYPE, SHAPE, NULL), (rc2, rows, cols)
        assert L.fq_last_error() != b""
        seen |= {rc, rc2}
    for _ in range(400):       # the same hostile sizes behind a served pair, so that the shape and argument checks are the ones that answer
        rows, cols, eps = rng.choice(INTS), rng.choice(INTS), rng.choice(FLOATS)
        xd, wd = rng.choice(SERVED)
        rc = L.fqn_rms_norm_fwd(*N4, rows, cols, eps, xd, wd, None)
        assert (rc == SHAPE) == bad_shape(rows, cols), (rc, rows, cols)
        bad_eps = not (eps >= 0 and math.isfinite(eps))
        assert rc == SHAPE or rc == (ARG if bad_eps else NULL), (rc, eps)
        rc2 = L.fqn_rms_norm_bwd(*N7, 0, rows, cols, xd, wd, None)
        assert rc2 == (SHAPE if bad_shape(rows, cols) else NULL), (rc2, rows, cols)
        seen |= {rc, rc2}
    for _ in range(400):       # the two size queries: 0 for what the entry points refuse, else the chunks of the rows
        rows, cols = rng.choice(INTS), rng.choice(INTS)
        parts, nbytes = L.fqn_rms_norm_bwd_parts(rows, cols), L.fqn_rms_norm_bwd_workspace_bytes(rows, cols)
        if bad_shape(rows, cols):
            assert parts == 0 and nbytes == 0, (rows, cols)
        else:
            assert 1 <= parts <= min(rows, 2048) and nbytes == parts * cols * 4, (rows, cols, parts, nbytes)
    assert seen == {DTYPE, SHAPE, ARG, NULL}          # never 0, never FQ_ERR_LAUNCH: NULL pointers are never launchable


# ---- the recipe, the reference helper and the fixture ------------------------------------------------------------------------------------------

def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "rms_norm.npz"))

    def load(key, dtype):
        a = z[key]
        t = torch.from_numpy(a.view(np.int16).copy()).view(dtype) if a.dtype == np.uint16 else torch.from_numpy(a.copy())
        assert t.dtype is dtype, (key, t.dtype)
        return t
    regular = int(z["regular"])
    for pair in z["pairs"]:
        xd, wd = (DT[p] for p in str(pair).split("_"))
        for h in z["hs"]:
            k = f"{pair}_h{h}_"
            yield (str(pair), int(h), regular, float(z[k + "eps"]), load(k + "x", xd), load(k + "w", wd), load(k + "g", wd), load(k + "y", wd),
                   load(k + "dx", xd), load(k + "dw", wd))


def same_or_both_nan(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) and torch.equal(bits(a.nan_to_num(0.0)), bits(b.nan_to_num(0.0)))


def test_the_fixture_holds_the_five_pairs_and_the_special_rows():
    cases = list(golden())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rms_norm.npz")) < 100 * 1024
    assert {c[0] for c in cases} == {"bf16_bf16", "f16_f16", "f32_f32", "bf16_f32", "f32_bf16"} and {c[1] for c in cases} == {7, 33, 256}
    for pair, h, regular, eps, x, w, g, y, dx, dw in cases:
        assert x.shape == y.shape == g.shape == dx.shape == (regular + 4, h) and w.shape == dw.shape == (h,)
        assert torch.isfinite(y[:regular]).all() and torch.isfinite(dx[:regular]).all() and torch.isfinite(dw).all()
        zero, nan, inf, big = (y[regular + i] for i in range(4))
        assert int(torch.count_nonzero(zero)) == 0 and nan.isnan().all()
        assert bool(inf[h - 1].isnan()) and int(torch.count_nonzero(inf[:h - 1])) == 0            # rstd = 0: NaN at the inf, 0 elsewhere
        if x.dtype is torch.float16:
            assert bool(big[0].isnan())                                                             # fp16 has no 1e20: a second inf
        else:
            assert int(torch.count_nonzero(big)) == 0 and torch.isfinite(x[regular + 3]).all()      # the sum overflows: rstd = 0, zeros


def test_recipe_of_the_chains_rstd_equals_the_chain_bit_for_bit():
    for pair, h, regular, eps, x, w, g, y, dx, dw in golden():
        got = R.recipe(x, w, R.chain_rstd(x, eps))
        assert got.dtype is y.dtype and same_or_both_nan(got, y), (pair, h)
        assert same_or_both_nan(R.chain(x, w, eps), y), (pair, h)
    for name, (x, w, g) in R.CASES().items():
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            xd, wd = x.to(dtype), w.to(dtype)
            assert torch.equal(bits(R.recipe(xd, wd, R.chain_rstd(xd))), bits(R.chain(xd, wd))), (name, dtype)
    g = torch.Generator().manual_seed(3)
    for h in (1, 2, 5, 688, 2049, 11008):
        for dtype in (torch.bfloat16, torch.float16, torch.float32):
            x, w = (torch.randn(4, h, generator=g) * 1.5).to(dtype), (1 + 0.1 * torch.randn(h, generator=g)).to(dtype)
            assert torch.equal(bits(R.recipe(x, w, R.chain_rstd(x))), bits(R.chain(x, w))), (h, dtype)


def test_the_backward_formula_equals_float64_autograd():
    for name, (x, w, g) in R.CASES().items():
        ref = R.ref64(x, w, g)
        dx, dw = R.formula64(x, w, g)
        sx, sw = float(ref[2].abs().max()), float(ref[3].abs().max())
        assert float((dx - ref[2]).abs().max()) <= 1e-15 * max(sx, 1.0) * x.shape[-1] ** 0.5, name
        assert float((dw - ref[3]).abs().max()) <= 1e-15 * max(sw, 1.0) * x.shape[0], name
    x, w, g = R.CASES()["randn_s1_h33"]
    dx, dw = R.formula64(x, w, g)
    ref = R.ref64(x, w, g)
    assert float((dx - ref[2]).abs().max()) <= 1e-15 and float((dw - ref[3]).abs().max()) <= 1e-15


def test_the_caps_are_the_size_of_an_eager_chains_error():
    """The caps are 4 x the chain's measures on the MI355X (tests/test_gpu_rms_norm.py checks that the chain sits within CAP / 4 there).
    Here the chain runs on ATen's CPU kernels, which sum in another order: its measures are of the caps' order of magnitude."""
    assert (R.RSTD_CAP, R.Y_CAP, R.DX_CAP, R.DW_CAP) == (4 * R.EAGER_E_RSTD, 4 * R.EAGER_E_Y, 4 * R.EAGER_C_DX, 4 * R.EAGER_C_DW)
    m = R.eager_measures("cpu")
    assert set(m) == set(R.CASES()) and len(m) == 14
    for x, w, g in R.CASES().values():
        assert torch.equal(x, x.bfloat16().float()) and torch.equal(w, w.bfloat16().float()) and torch.equal(g, g.bfloat16().float())
    worst = [max(v[i] for v in m.values()) for i in range(4)]
    print({k: tuple(round(t, 3) for t in v) for k, v in m.items()})
    for got, cap in zip(worst, (R.RSTD_CAP, R.Y_CAP, R.DX_CAP, R.DW_CAP)):
        assert cap / 16 < got < cap, (worst, cap)


def test_the_measures_see_an_error_of_their_size():
    x, w, g = R.CASES()["randn_s1_h256"]
    ref = R.ref64(x, w, g)
    y64, rstd64, dx64, dw64 = ref[:4]
    assert R.e_rstd(rstd64, ref) == 0.0 and R.e_y(y64, w, ref) == 0.0 and R.c_dx(dx64, ref) == 0.0 and R.c_dw(dw64, g, ref) == 0.0
    assert R.e_rstd(rstd64 * (1 + 100 * R.UNIT), ref) == pytest.approx(100, rel=1e-6) and 100 > R.RSTD_CAP
    for wrong, measure, cap in ((y64.clone(), lambda t: R.e_y(t.float(), w, ref), R.Y_CAP), (dx64.clone(), lambda t: R.c_dx(t.float(), ref), R.DX_CAP)):
        wrong[1, 7] *= 1 + 2.0 ** -12         # one element, 4096 fp32 ulp off
        assert measure(wrong) > cap
    wrong = dw64.clone()
    wrong[5] *= 1 + 2.0 ** -10
    assert R.c_dw(wrong.float(), g, ref) > R.DW_CAP
    assert R.c_dx(dx64.bfloat16(), ref) == 0.0 and R.c_dw(dw64.half(), g, ref) == 0.0        # the output rounding is allowed for ...
    assert R.c_dx(dx64.bfloat16().float(), ref) > R.DX_CAP                                   # ... only where the dtype has it


# ---- CPU tensors -----------------------------------------------------------------------------------------------------------------------------

def test_cpu_tensors_are_refused_by_default_and_served_bit_for_bit_after_the_opt_in():
    from llm_qat_amd import cpu_tensors
    was = cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(False)
        x, w, _ = R.CASES()["randn_s1_h33"]
        for f in (lambda: norm.rms_norm(x, w), lambda: norm.RMSNorm(33)(x)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f()
        llm_qat_amd.allow_cpu_tensors(True)
        before = dict(ops.norm_counts)
        for pair, h, regular, eps, x, w, g, y, dx, dw in golden():
            xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            got = norm.rms_norm(xr, wr, eps)
            assert got.dtype is y.dtype and same_or_both_nan(got, y), (pair, h)
            (gx,) = torch.autograd.grad(got, xr, g)
            assert gx.dtype is dx.dtype and same_or_both_nan(gx, dx), (pair, h)
            m = norm.RMSNorm(h, eps)
            m.weight.data = w.clone()
            (gw,) = torch.autograd.grad(m(x[:regular]), m.weight, g[:regular])
            assert gw.dtype is dw.dtype and torch.equal(bits(gw), bits(dw)), (pair, h)
        assert ops.norm_counts == before                     # no launch, no copy: torch ops
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


# ---- the class, install(), convert(), the package surface ---------------------------------------------------------------------------------------

class StockNorm(torch.nn.Module):
    """the shape of LlamaRMSNorm (the reference's and Hugging Face's): a 1-D weight and variance_epsilon"""

    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        return R.chain(hidden_states, self.weight, self.variance_epsilon)


def test_the_class_has_the_references_constructor_attributes_and_checkpoints():
    import inspect
    assert list(inspect.signature(norm.RMSNorm.__init__).parameters) == ["self", "hidden_size", "eps"]
    assert inspect.signature(norm.RMSNorm.__init__).parameters["eps"].default == 1e-6
    m = norm.RMSNorm(33, eps=1e-5)
    assert isinstance(m, torch.nn.Module) and isinstance(m.weight, torch.nn.Parameter) and m.variance_epsilon == 1e-5
    assert m.weight.shape == (33,) and bool((m.weight == 1).all()) and list(m.state_dict()) == ["weight"] and "33" in repr(m)
    stock = StockNorm(33)
    with torch.no_grad():
        stock.weight.copy_(torch.randn(33))
    assert m.load_state_dict(stock.state_dict()).missing_keys == [] and torch.equal(m.weight, stock.weight)
    back = StockNorm(33)
    back.load_state_dict(m.state_dict())
    assert torch.equal(back.weight, stock.weight)


def test_install_replaces_the_modules_attribute_and_returns_the_old_one():
    ns = types.ModuleType("modeling_stand_in")
    ns.LlamaRMSNorm = StockNorm
    assert norm.install(ns) is StockNorm and ns.LlamaRMSNorm is norm.RMSNorm
    ns.LlamaRMSNorm = StockNorm                                # the undo
    assert norm.install(ns) is StockNorm and norm.install(ns) is norm.RMSNorm
    bare = types.ModuleType("bare")
    assert norm.install(bare) is None and bare.LlamaRMSNorm is norm.RMSNorm
    for wrong in (object(), {"LlamaRMSNorm": 1}, StockNorm):
        with pytest.raises(TypeError, match="module object"):
            norm.install(wrong)


def test_convert_swaps_the_norms_in_place_and_leaves_everything_else_alone():
    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.input_layernorm = StockNorm(16, 1e-5)
            self.q_proj = QuantizeLinear(16, 16, bias=False, w_bits=4, a_bits=8)
            self.head = torch.nn.Linear(16, 4)
            self.ln = torch.nn.LayerNorm(16)
            self.layers = torch.nn.ModuleList([StockNorm(16), norm.RMSNorm(16)])
    model = Block().eval()
    params = dict(model.named_parameters())
    kept = (model.q_proj, model.head, model.ln, model.layers[1])
    assert norm.convert(model) == 2
    assert isinstance(model.input_layernorm, norm.RMSNorm) and isinstance(model.layers[0], norm.RMSNorm)
    assert model.input_layernorm.variance_epsilon == 1e-5 and not model.input_layernorm.training
    assert (model.q_proj, model.head, model.ln, model.layers[1]) == kept and type(model.q_proj) is QuantizeLinear
    after = dict(model.named_parameters())
    assert list(after) == list(params) and all(after[k] is params[k] for k in params)       # the Parameter objects are kept
    assert norm.convert(model) == 0
    with pytest.raises(TypeError, match="torch.nn.Module"):
        norm.convert([model])


def test_the_public_names_live_in_the_submodule():
    assert llm_qat_amd.norm is norm and norm.__all__ == ["rms_norm", "RMSNorm", "install", "convert"]
    for name in ["norm"] + norm.__all__:
        assert name not in llm_qat_amd.__all__, name
    assert not hasattr(llm_qat_amd, "rms_norm") and not hasattr(llm_qat_amd, "RMSNorm")
    assert llm_qat_amd.__all__[-2:] == ["MXLinear", "convert_to_mx_inference"] and len(llm_qat_amd.__all__) == len(set(llm_qat_amd.__all__))
    assert set(ops.norm_counts) == {"fwd_launch", "bwd_launch", "copy_route"}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "llm_qat_amd.norm" in text and "install(" in text and "convert(" in text


# ---- the compiled ops' fake implementations ----------------------------------------------------------------------------------------------------

def test_fake_ops_shapes_and_dtypes_on_meta_tensors():
    assert str(compiled.rms_norm_fwd_op._opoverload._schema) == "llmqat_amd::rms_norm_fwd(Tensor x, Tensor weight, float eps, bool need_stats) -> (Tensor, Tensor)"
    assert str(compiled.rms_norm_bwd_op._opoverload._schema) == \
        "llmqat_amd::rms_norm_bwd(Tensor g, Tensor x, Tensor weight, Tensor rstd, bool need_dx, bool need_dw) -> (Tensor, Tensor)"
    pairs = [(a, b) for a in DT.values() for b in DT.values() if a is b or torch.float32 in (a, b)]
    assert len(pairs) == 7
    for xd, wd in pairs:
        for shape in ((6, 515), (2, 3, 4096), (33,)):
            x, w = torch.empty(shape, dtype=xd, device="meta"), torch.empty(shape[-1], dtype=wd, device="meta")
            y, none = torch.ops.llmqat_amd.rms_norm_fwd(x, w, 1e-6, False)
            assert tuple(y.shape) == shape and none.numel() == 0 and none.dtype is torch.float32       # no stats: nothing to write
            y, rstd = torch.ops.llmqat_amd.rms_norm_fwd(x, w, 1e-6, True)
            rows = x.numel() // shape[-1]
            assert y.device.type == "meta" and tuple(y.shape) == shape and y.dtype is wd
            assert tuple(rstd.shape) == (rows,) and rstd.dtype is torch.float32
            dx, dw = torch.ops.llmqat_amd.rms_norm_bwd(y, x, w, rstd, True, True)
            assert tuple(dx.shape) == shape and dx.dtype is xd and dx.is_contiguous() and tuple(dw.shape) == (shape[-1],) and dw.dtype is wd
            dx, dw = torch.ops.llmqat_amd.rms_norm_bwd(y, x, w, rstd, True, False)
            assert tuple(dx.shape) == shape and dw.numel() == 0
            dx, dw = torch.ops.llmqat_amd.rms_norm_bwd(y, x, w, rstd, False, True)
            assert dx.numel() == 0 and tuple(dw.shape) == (shape[-1],)
    x, w = torch.empty(4, 8, dtype=torch.float64, device="meta"), torch.empty(8, device="meta")
    with pytest.raises(TypeError, match="not served"):
        torch.ops.llmqat_amd.rms_norm_fwd(x, w, 1e-6, True)
    with pytest.raises(ValueError, match="shape mismatch"):
        torch.ops.llmqat_amd.rms_norm_fwd(x.float(), torch.empty(9, device="meta"), 1e-6, True)


# ---- Python argument refusals (all before any launch; the device check is the last of them, so CPU tensors reach the others) -----------------

def test_python_argument_refusals():
    x, w = torch.zeros(2, 3, 8), torch.ones(8)
    before = dict(ops.norm_counts)
    for f in (norm.rms_norm, ops.rms_norm_forward):
        with pytest.raises(TypeError, match="float64 is not served"):
            f(x.double(), w)
        with pytest.raises(TypeError, match="float64 is not served"):
            f(x, w.double())
        with pytest.raises(TypeError, match="torch.int32 is not served"):
            f(x.int(), w)
        with pytest.raises(TypeError, match="pair") as e:
            f(x.bfloat16(), w.half())
        assert "exactly one" in str(e.value)
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(x, None)
        with pytest.raises(TypeError, match="eps is a number"):
            f(x, w, "1e-6")
        for eps in (-1e-6, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite and not negative"):
                f(x, w, eps)
        with pytest.raises(ValueError, match="1-D"):
            f(x, w.reshape(1, 8))
        with pytest.raises(ValueError, match="shape mismatch"):
            f(x, torch.ones(7))
        with pytest.raises(ValueError, match="empty"):
            f(x[:0], w)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.rms_norm_forward(x, w)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.rms_norm_backward(x, x, w, torch.zeros(6))
    assert ops.norm_counts == before
