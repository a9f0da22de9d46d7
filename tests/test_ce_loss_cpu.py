"""CPU tier of the fused language-model loss: the fqc_ header and its binding, every refusal of the two entry points
in the order the header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers below are never
dereferenced), the contract's formula and the reference helper checked against F.cross_entropy in float64, the shift identity, the
CPU-tensor route, the CrossEntropyLoss class, install(), the package surface, the compiled ops' fake implementations and the Python
argument refusals."""
import ctypes
import math
import os
import random
import re
import types

import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd
from llm_qat_amd import _lib, compiled, distill, lm_loss, ops

import ce_loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, LAB, LSE, RL, LO, NV, G, GX = 0x1000, 0x2008, 0x3004, 0x4004, 0x5004, 0x6008, 0x7004, 0x8002      # never dereferenced
F32, BF16, F16, F64 = 0, 1, 2, 3
MEAN, SUM = 0, 1
DTYPE, SHAPE, NULL, LAUNCH, ARG, UNSUPPORTED = -1, -3, -4, -6, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 32000, 32001, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]


def fwd(*a):
    L = _lib.lib()
    rc = L.fqc_ce_fwd(*a, None)
    return rc, L.fq_last_error().decode()


def bwd(*a):
    L = _lib.lib()
    rc = L.fqc_ce_bwd(*a, None)
    return rc, L.fq_last_error().decode()


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_ce_header_names_equal_ce_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_ce.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fqc_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.CE_EXPORTS) == {"fqc_ce_fwd", "fqc_ce_bwd"}
    assert not re.findall(r"\bfq[tsil]?_[a-z0-9_]+\s*\(", src)      # nothing of the five other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    others = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS) | set(_lib.INFER_EXPORTS) | set(_lib.LOSS_EXPORTS)
    assert not set(_lib.CE_EXPORTS) & others
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for f in (L.fqc_ce_fwd, L.fqc_ce_bwd):
        assert f.argtypes == [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i64, i32, i32, vp] and f.restype is i32
    assert (_lib.CE_MEAN, _lib.CE_SUM) == (0, 1) and "#define FQC_REDUCTION_MEAN 0" in src and "#define FQC_REDUCTION_SUM 1" in src


def test_the_build_lists_the_new_unit_and_headers():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_ce_loss.hip", "fq_ce_loss.h", "fq_loss_rows.h", "fq_rows.h", "llmqat_fakequant_ce.h"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

N6 = (None,) * 6
FWD_REFUSALS = [
    # (logits, labels, row_lse, row_loss, loss, n_valid, rows, cols, seq_len, shift, ignore_index, reduction, dtype), code, part of the message
    (N6 + (-1, -1, 0, 7, -100, 9, 9), DTYPE, "unknown dtype"),
    (N6 + (-1, -1, 0, 7, -100, 9, -1), DTYPE, "unknown dtype"),
    (N6 + (-1, -1, 0, 7, -100, 9, F64), DTYPE, "float64"),
    (N6 + (-3, 8, 0, 7, -100, 9, BF16), SHAPE, "negative shape"),
    (N6 + (3, -8, 0, 7, -100, 9, F16), SHAPE, "negative shape"),
    (N6 + (0, 8, 0, 7, -100, 9, F32), SHAPE, "empty shape"),
    (N6 + (3, 0, 0, 7, -100, 9, BF16), SHAPE, "empty shape"),
    (N6 + (2 ** 62, 2 ** 40, 0, 7, -100, 9, BF16), SHAPE, "overflows"),
    (N6 + (7, 8, 3, 1, -100, 9, BF16), SHAPE, "not whole sequences"),
    (N6 + (6, 8, 3, 2, -100, 9, BF16), ARG, "shift=2"),
    (N6 + (6, 8, 3, -1, -100, 9, F32), ARG, "shift=-1"),
    (N6 + (6, 8, 0, 1, -100, 9, F32), ARG, "unknown reduction"),           # the reduction comes before seq_len
    (N6 + (6, 8, 3, 1, -100, 2, F16), ARG, "unknown reduction"),
    (N6 + (6, 8, 0, 1, -100, SUM, BF16), ARG, "seq_len=0"),
    (N6 + (6, 8, -3, 0, -100, MEAN, BF16), ARG, "seq_len=-3"),               # also without the shift
    ((None, LAB, LSE, RL, LO, NV, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, None, LSE, RL, LO, NV, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, None, LO, NV, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, RL, None, NV, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, RL, LO, None, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    (N6 + (2 ** 40, 32000, 2 ** 20, 1, -100, SUM, F16), NULL, "NULL"),                                 # the pointers come before the grid
    ((X, LAB, None, RL, LO, NV, 2 ** 33, 2048, 2 ** 11, 1, -100, MEAN, BF16), UNSUPPORTED, "exceed one launch's grid"),    # row_lse may be NULL
    ((X, LAB, LSE, RL, LO, NV, 2 ** 34, 8, 1, 0, -100, SUM, F32), UNSUPPORTED, "exceed one launch's grid"),
]
BWD_REFUSALS = [
    # (logits, labels, row_lse, n_valid, grad_loss, grad_logits, rows, cols, seq_len, shift, ignore_index, reduction, dtype), code, part of the message
    (N6 + (-1, -1, 0, 7, -100, 9, 9), DTYPE, "unknown dtype"),
    (N6 + (-1, -1, 0, 7, -100, 9, F64), DTYPE, "float64"),
    (N6 + (-3, 8, 0, 7, -100, 9, BF16), SHAPE, "negative shape"),
    (N6 + (0, 8, 0, 7, -100, 9, F32), SHAPE, "empty shape"),
    (N6 + (3, 0, 0, 7, -100, 9, F16), SHAPE, "empty shape"),
    (N6 + (2 ** 62, 2 ** 40, 0, 7, -100, 9, BF16), SHAPE, "overflows"),
    (N6 + (7, 8, 3, 1, -100, 9, BF16), SHAPE, "not whole sequences"),
    (N6 + (6, 8, 3, 2, -100, 9, BF16), ARG, "shift=2"),
    (N6 + (6, 8, 0, 1, -100, 9, F32), ARG, "unknown reduction"),
    (N6 + (6, 8, 0, 1, -100, SUM, BF16), ARG, "seq_len=0"),
    ((None, LAB, LSE, NV, G, GX, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, None, LSE, NV, G, GX, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, None, NV, G, GX, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, None, G, GX, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, NV, None, GX, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, NV, G, None, 6, 8, 3, 1, -100, MEAN, BF16), NULL, "NULL"),
    ((X, LAB, LSE, NV, G, X, 6, 8, 3, 1, -100, MEAN, BF16), ARG, "in-place"),
    ((X, LAB, LSE, NV, G, X, 2 ** 34, 8, 1, 0, -100, SUM, F32), ARG, "in-place"),                       # the aliasing comes before the grid
    ((X, LAB, LSE, NV, G, GX, 2 ** 34, 8, 1, 0, -100, SUM, F32), UNSUPPORTED, "exceed one launch's grid"),
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


def test_every_served_dtype_shift_and_reduction_passes_the_first_checks():
    for dtype in (F32, BF16, F16):
        for shift in (0, 1):
            for red in (MEAN, SUM):
                assert fwd(*N6, 6, 32001, 3, shift, -100, red, dtype)[0] == NULL
                assert bwd(*N6, 6, 32001, 3, shift, -100, red, dtype)[0] == NULL
    assert fwd(*N6, 7, 8, 3, 0, -100, MEAN, BF16)[0] == NULL          # without the shift, seq_len need not divide the rows


def test_fuzz_never_reaches_a_launch():
    rng = random.Random(23)
    L = _lib.lib()
    seen = set()
    clamp = lambda v: max(-(2 ** 31), min(2 ** 31 - 1, v))      # noqa: E731
    for f in (L.fqc_ce_fwd, L.fqc_ce_bwd):
        for _ in range(400):
            rows, cols, seq = rng.choice(INTS), rng.choice(INTS), rng.choice(INTS)
            rc = f(*N6, rows, cols, seq, clamp(rng.choice(INTS)), rng.choice(INTS), clamp(rng.choice(INTS)), clamp(rng.choice(INTS)), None)
            assert rc in (DTYPE, SHAPE, ARG, NULL), (rc, rows, cols, seq)
            assert L.fq_last_error() != b""
            seen.add(rc)
        for _ in range(600):       # the same hostile sizes behind a valid dtype, so that the shape and argument checks are the ones that answer
            rows, cols, seq = rng.choice(INTS), rng.choice(INTS), rng.choice(INTS)
            shift, red = rng.choice((0, 1, 1, 2, -1)), rng.choice((0, 1, 1, 2))
            rc = f(*N6, rows, cols, seq, shift, rng.choice(INTS), red, rng.randrange(3), None)
            assert rc in (SHAPE, ARG, NULL), (rc, rows, cols, seq)
            bad_shape = rows <= 0 or cols <= 0 or rows * cols > (2 ** 63 - 1) // 4 or (shift == 1 and seq > 0 and rows % seq != 0)
            assert (rc == SHAPE) == bad_shape, (rc, rows, cols, seq, shift)
            assert rc == SHAPE or (rc == ARG) == (shift not in (0, 1) or red not in (0, 1) or seq <= 0), (rc, seq, shift, red)
            seen.add(rc)
    assert seen == {DTYPE, SHAPE, ARG, NULL}          # never 0, never FQ_ERR_LAUNCH: NULL pointers are never launchable


# ---- the contract's formula and the reference helper, on their own ------------------------------------------------------------------------------

def _small(rows, v, seed, ignored=()):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, v, generator=g) * 3
    y = torch.randint(0, v, (rows,), generator=g)
    for r in ignored:
        y[r] = R.IGNORE
    return x, y


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_the_formula_equals_cross_entropy_and_its_autograd_gradient_in_float64(reduction):
    for name, (x, y) in list(R.CASES().items()) + [("small", _small(6, 33, 1, (0, 4))), ("none_ignored", _small(5, 7, 2))]:
        loss64, d64, *_ = R.ref64(x, y, reduction)
        loss, grad, row_loss, n = R.formula64(x, y, False, reduction)
        assert n == int((y != R.IGNORE).sum()) and n >= 1
        assert abs(float(loss - loss64)) <= 1e-13 * abs(float(loss64)), name
        assert float((grad - d64).abs().max()) <= 1e-14, name
        assert (grad[y == R.IGNORE] == 0).all() and (row_loss[y == R.IGNORE] == 0).all()
        want_rows = F.cross_entropy(x.double(), y, ignore_index=R.IGNORE, reduction="none")
        assert float((row_loss - want_rows).abs().max()) <= 1e-12, name


def test_no_valid_row_is_nan_under_mean_and_zero_under_sum():
    x, y = _small(4, 9, 3, (0, 1, 2, 3))
    assert math.isnan(float(F.cross_entropy(x.double(), y, reduction="mean"))) and float(F.cross_entropy(x.double(), y, reduction="sum")) == 0.0
    loss, grad, _, n = R.formula64(x, y, False, "mean")
    assert n == 0 and math.isnan(float(loss)) and int(torch.count_nonzero(grad)) == 0
    loss, grad, _, n = R.formula64(x, y, False, "sum")
    assert n == 0 and float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_the_shift_identity(reduction):
    """the formula on the unshifted [B, T, V] pair with shift equals the sliced-and-flattened call; the gradient's last position is zero"""
    g = torch.Generator().manual_seed(4)
    for shape in ((2, 5, 33), (3, 4, 17), (1, 1, 8), (2, 2, 3, 9)):
        x = torch.randn(shape, generator=g) * 3
        lab = torch.randint(0, shape[-1], shape[:-1], generator=g)
        lab[..., 0] = R.IGNORE            # the first label is never used: it must not matter
        if shape[-2] > 2:
            lab[0, ..., 2] = R.IGNORE
        loss, grad, _, n = R.formula64(x, lab, True, reduction)
        xs, ys = x[..., :-1, :].reshape(-1, shape[-1]), lab[..., 1:].reshape(-1)
        assert n == int((ys != R.IGNORE).sum())
        assert int(torch.count_nonzero(grad[..., -1, :])) == 0
        if n == 0:
            assert math.isnan(float(loss)) if reduction == "mean" else float(loss) == 0.0
            continue
        want, wgrad, _, _ = R.formula64(xs, ys, False, reduction)
        assert float(loss) == pytest.approx(float(want), rel=1e-14)
        assert torch.equal(grad[..., :-1, :].reshape(-1, shape[-1]), wgrad)
        x64 = x.double().requires_grad_(True)
        ref = F.cross_entropy(x64[..., :-1, :].contiguous().view(-1, shape[-1]), lab[..., 1:].contiguous().view(-1), reduction=reduction)
        (rgrad,) = torch.autograd.grad(ref, x64)
        assert float(loss) == pytest.approx(float(ref.detach()), rel=1e-13) and float((grad - rgrad).abs().max()) <= 1e-14
        if reduction == "mean":
            assert float(R.chain(x.double(), lab)) == float(ref.detach())


def test_the_caps_are_the_size_of_an_eager_chains_error():
    """The caps are 4 x the chain's measures on the MI355X (tests/test_gpu_ce_loss.py checks that the chain sits within CAP / 4 there).
    Here the chain runs on ATen's CPU kernels, which sum in another order: its measures are of the caps' order of magnitude."""
    assert R.LOSS_CAP == 4 * R.EAGER_E_LOSS and R.GRAD_CAP == 4 * R.EAGER_C_GRAD
    m = R.eager_measures("cpu")
    assert set(m) == set(R.CASES()) and len(m) == 7
    for x, y in R.CASES().values():
        ignored = int((y == R.IGNORE).sum())
        assert x.shape[0] == 8 and ignored == 2 and torch.equal(x, x.bfloat16().float())
    worst_loss, worst_grad = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print({k: (round(a, 3), round(b, 2)) for k, (a, b) in m.items()})
    assert R.LOSS_CAP / 16 < worst_loss < 16 * R.LOSS_CAP and R.GRAD_CAP / 16 < worst_grad < 16 * R.GRAD_CAP, (worst_loss, worst_grad)


def test_the_measures_see_an_error_of_their_size():
    x, y = R.CASES()["randn_s3_v4099"]
    ref = R.ref64(x, y)
    loss64, d64 = ref[0], ref[1]
    n = R.e_loss(loss64 * 0, x, y, ref=ref) * R.UNIT / float(loss64)            # = 1 / N
    assert R.e_loss(loss64, x, y, ref=ref) == 0.0 and R.c_grad(d64, x, y, ref=ref) == 0.0
    assert R.e_loss(loss64 + 100 * R.UNIT / n, x, y, ref=ref) == pytest.approx(100, rel=1e-6) and 100 > R.LOSS_CAP
    wrong = d64.clone()
    wrong[1, int(ref[4][1].argmax())] *= 1 + 2.0 ** -10       # one element, 16384 fp32 ulp off
    assert R.c_grad(wrong, x, y, ref=ref) > R.GRAD_CAP
    wrong = d64.clone()
    wrong[2, 5] = 1.0                                          # an ignored row is outside the measure (the tests check its bytes)
    assert R.c_grad(wrong, x, y, ref=ref) == 0.0
    assert R.c_grad(d64.bfloat16(), x, y, torch.bfloat16, ref=ref) == 0.0                    # the output rounding is allowed for ...
    assert R.c_grad(d64.bfloat16(), x, y, torch.float32, ref=ref) > R.GRAD_CAP               # ... only where the dtype has it
    assert R.c_grad(0.37 * d64, x, y, g=0.37, ref=ref) < 1e-3


# ---- CPU tensors -----------------------------------------------------------------------------------------------------------------------------

def test_cpu_tensors_are_refused_by_default_and_served_after_the_opt_in():
    from llm_qat_amd import cpu_tensors
    was = cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(False)
        x, y = R.CASES()["randn_s30_v33"]
        for f in (lm_loss.cross_entropy, lm_loss.causal_lm_loss, lm_loss.CrossEntropyLoss()):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                f(x, y)
        llm_qat_amd.allow_cpu_tensors(True)
        before = dict(ops.ce_counts)
        # 1e-6 relative to F.cross_entropy in fp32 is a bound on ATen's own rounding: half an ulp of lse, which multiplies every
        # probability, is 2^-21 = 4.8e-7 for |lse| < 16, so the comparison takes the cases with sigma <= 3 (|lse| < 14); at sigma = 30
        # (|lse| about 64) ATen's fp32 result is itself 3e-6 from float64, and that case is checked against float64 below instead
        for name in ("randn_s1_v4099", "randn_s3_v4099", "randn_s30_v33"):
            x, y = R.CASES()[name]
            for reduction in ("mean", "sum") if name != "randn_s30_v33" else ():
                xd = x.clone().requires_grad_(True)
                loss = lm_loss.cross_entropy(xd, y, reduction=reduction)
                assert loss.dtype is torch.float32 and loss.dim() == 0
                (0.37 * loss).backward()
                xe = x.clone().requires_grad_(True)
                want = F.cross_entropy(xe, y, reduction=reduction)
                (0.37 * want).backward()
                assert float(loss) == pytest.approx(float(want), rel=1e-6), (name, reduction)
                assert float((xd.grad - xe.grad).abs().max()) <= 1e-6 * float(xe.grad.abs().max()), (name, reduction)
                assert int(torch.count_nonzero(xd.grad[y == R.IGNORE])) == 0
            for dtype in (torch.bfloat16, torch.float16):
                xd = x.to(dtype).requires_grad_(True)
                lm_loss.cross_entropy(xd, y).backward()
                assert xd.grad.dtype is dtype and xd.grad.shape == xd.shape
                assert R.c_grad(xd.grad, xd, y, dtype) <= R.GRAD_CAP
        g = torch.Generator().manual_seed(6)                    # the shift, and the class
        x3 = (torch.randn(2, 5, 33, generator=g) * 3).requires_grad_(True)
        lab = torch.randint(0, 33, (2, 5), generator=g)
        lab[1, 3] = R.IGNORE
        loss = lm_loss.causal_lm_loss(x3, lab)
        loss.backward()
        xe = x3.detach().clone().requires_grad_(True)
        want = R.chain(xe, lab)
        want.backward()
        assert float(loss) == pytest.approx(float(want), rel=1e-6) and float((x3.grad - xe.grad).abs().max()) <= 1e-6 * float(xe.grad.abs().max())
        assert int(torch.count_nonzero(x3.grad[:, -1])) == 0
        assert float(lm_loss.CrossEntropyLoss(reduction="sum")(x, y)) == pytest.approx(float(F.cross_entropy(x, y, reduction="sum")), rel=1e-6)
        bad = x.clone()                                          # an ignored row is never looked at; a label out of range is NaN, not a fault
        bad[2] = float("nan")
        bd = bad.requires_grad_(True)
        loss = lm_loss.cross_entropy(bd, y)
        loss.backward()
        assert float(loss) == pytest.approx(float(F.cross_entropy(x, y)), rel=1e-6) and torch.isfinite(bd.grad).all()
        yo = y.clone()
        yo[0] = 33
        xo = x.clone().requires_grad_(True)
        loss = lm_loss.cross_entropy(xo, yo)
        loss.backward()
        assert math.isnan(float(loss)) and torch.isnan(xo.grad[0]).all() and torch.isfinite(xo.grad[1:]).all()
        none = torch.full_like(y, R.IGNORE)
        assert math.isnan(float(lm_loss.cross_entropy(x, none))) and float(lm_loss.cross_entropy(x, none, reduction="sum")) == 0.0
        assert ops.ce_counts == before                       # no launch, no copy: torch ops
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


# ---- the class, install(), the package surface ----------------------------------------------------------------------------------------------------

def test_the_class_takes_torchs_constructor_and_refuses_what_is_not_served():
    import inspect
    ours = list(inspect.signature(lm_loss.CrossEntropyLoss.__init__).parameters)
    assert ours == list(inspect.signature(torch.nn.CrossEntropyLoss.__init__).parameters)
    m = lm_loss.CrossEntropyLoss()
    assert isinstance(m, torch.nn.Module) and (m.ignore_index, m.reduction) == (-100, "mean")
    m = lm_loss.CrossEntropyLoss(None, None, -1, None, "sum", 0.0)
    assert (m.ignore_index, m.reduction) == (-1, "sum") and "sum" in repr(m)
    for kwargs, text in (({"weight": torch.ones(3)}, "class weights"), ({"label_smoothing": 0.1}, "label_smoothing"),
                         ({"size_average": True}, "size_average"), ({"reduce": False}, "size_average / reduce"), ({"reduction": "none"}, "'none'")):
        with pytest.raises(NotImplementedError, match=text) as e:
            lm_loss.CrossEntropyLoss(**kwargs)
        assert "'mean' or 'sum'" in str(e.value)             # the message names what is served
    with pytest.raises(TypeError, match="ignore_index"):
        lm_loss.CrossEntropyLoss(ignore_index=1.5)


def test_install_replaces_the_modules_attribute_and_returns_the_old_one():
    ns = types.ModuleType("modeling_stand_in")
    ns.CrossEntropyLoss = torch.nn.CrossEntropyLoss
    assert lm_loss.install(ns) is torch.nn.CrossEntropyLoss
    assert ns.CrossEntropyLoss is lm_loss.CrossEntropyLoss
    ns.CrossEntropyLoss = torch.nn.CrossEntropyLoss           # the undo
    assert lm_loss.install(ns) is torch.nn.CrossEntropyLoss and lm_loss.install(ns) is lm_loss.CrossEntropyLoss
    bare = types.ModuleType("bare")
    assert lm_loss.install(bare) is None and bare.CrossEntropyLoss is lm_loss.CrossEntropyLoss
    for wrong in (object(), {"CrossEntropyLoss": 1}, torch.nn.CrossEntropyLoss):
        with pytest.raises(TypeError, match="module object"):
            lm_loss.install(wrong)


def test_the_public_names_live_in_the_submodule():
    assert llm_qat_amd.lm_loss is lm_loss and lm_loss.__all__ == ["cross_entropy", "causal_lm_loss", "CrossEntropyLoss", "install"]
    for name in ["lm_loss"] + lm_loss.__all__[:3]:
        assert name not in llm_qat_amd.__all__, name
    assert not hasattr(llm_qat_amd, "causal_lm_loss") and not hasattr(llm_qat_amd, "cross_entropy")
    assert llm_qat_amd.__all__[-2:] == ["MXLinear", "convert_to_mx_inference"] and len(llm_qat_amd.__all__) == len(set(llm_qat_amd.__all__))
    assert distill.__all__ == ["kd_kl_loss", "install"]
    assert set(ops.ce_counts) == {"fwd_launch", "bwd_launch", "copy_route"}
    for f in (lm_loss.cross_entropy, lm_loss.causal_lm_loss):
        assert "fp32" in f.__doc__ and "autocast" in f.__doc__ and "16 bits" in f.__doc__
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lm_loss" in text and "causal_lm_loss(" in text and "install(" in text


# ---- the compiled ops' fake implementations ----------------------------------------------------------------------------------------------------

def test_fake_ops_shapes_and_dtypes_on_meta_tensors():
    assert str(compiled.ce_fwd_op._opoverload._schema) == \
        "llmqat_amd::ce_fwd(Tensor logits, Tensor labels, bool shift, SymInt ignore_index, str reduction) -> (Tensor, Tensor, Tensor)"
    assert str(compiled.ce_bwd_op._opoverload._schema) == \
        ("llmqat_amd::ce_bwd(Tensor logits, Tensor labels, Tensor row_lse, Tensor n_valid, Tensor grad_loss, bool shift, SymInt ignore_index, "
         "str reduction) -> Tensor")
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for shape in ((6, 515), (2, 3, 32001), (2, 2, 2, 33)):
            x = torch.empty(shape, dtype=dtype, device="meta")
            y = torch.empty(shape[:-1], dtype=torch.int64, device="meta")
            for shift in (False, True):
                loss, lse, n = torch.ops.llmqat_amd.ce_fwd(x, y, shift, -100, "mean")
                rows = x.numel() // shape[-1]
                assert loss.device.type == "meta" and loss.shape == () and loss.dtype is torch.float32
                assert tuple(lse.shape) == (rows,) and lse.dtype is torch.float32 and tuple(n.shape) == (1,) and n.dtype is torch.int64
                g = torch.ops.llmqat_amd.ce_bwd(x, y, lse, n, loss, shift, -100, "sum")
                assert tuple(g.shape) == shape and g.dtype is dtype and g.is_contiguous()
    x, y = torch.empty(4, 8, dtype=torch.float64, device="meta"), torch.empty(4, dtype=torch.int64, device="meta")
    with pytest.raises(TypeError, match="not served"):
        torch.ops.llmqat_amd.ce_fwd(x, y, False, -100, "mean")
    with pytest.raises(ValueError, match="shape mismatch"):
        torch.ops.llmqat_amd.ce_fwd(x.float(), torch.empty(5, dtype=torch.int64, device="meta"), False, -100, "mean")


# ---- Python argument refusals (all before any launch; the device check is the last of them, so CPU tensors reach the others) -----------------

def test_python_argument_refusals():
    x, y = torch.zeros(2, 3, 8), torch.zeros(2, 3, dtype=torch.int64)
    before = dict(ops.ce_counts)
    for f in (lm_loss.cross_entropy, lm_loss.causal_lm_loss, ops.ce_forward):
        with pytest.raises(TypeError, match="float64 is not served"):
            f(x.double(), y)
        with pytest.raises(TypeError, match="torch.int32 is not served"):
            f(x.int(), y)
        with pytest.raises(TypeError, match="labels of dtype torch.int32 are not served"):
            f(x, y.int())
        with pytest.raises(TypeError, match="probability targets") as e:
            f(x, torch.zeros(2, 3, 8))
        assert "'mean' or 'sum'" in str(e.value)
        with pytest.raises(ValueError, match="shape mismatch"):
            f(x, y[:, :2])
        with pytest.raises(ValueError, match="at least two dimensions"):
            f(x[0, 0], y[0, 0])
        with pytest.raises(ValueError, match="empty"):
            f(x[:, :0], y[:, :0])
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(x, None)
        with pytest.raises(TypeError, match="ignore_index is an int"):
            f(x, y, ignore_index=1.0)
        with pytest.raises(ValueError, match="reduction='none' is not served") as e:
            f(x, y, reduction="none")
        assert "'mean' or 'sum'" in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.ce_forward(x, y)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.ce_backward(x, y, torch.zeros(6), torch.ones(1, dtype=torch.int64), torch.ones(()))
    assert ops.ce_counts == before
