"""CPU tier of the fused distillation loss: the fql_ header and its binding, every refusal of the two entry points in
the order the header states (validation precedes every HIP call, so no GPU is needed: the non-NULL pointers below are never dereferenced),
the reference helper checked on its own, install(), the package surface, the CPU-tensor route, the compiled ops' fake implementations and
the Python argument refusals."""
import ctypes
import math
import os
import random
import re

import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, compiled, distill, ops

import kd_loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, T, ST, RL, LO, G, GS = 0x1000, 0x2000, 0x3004, 0x4004, 0x5004, 0x6004, 0x7002      # never dereferenced; none needs an alignment
F32, BF16, F16, F64 = 0, 1, 2, 3
DTYPE, SHAPE, NULL, LAUNCH, ARG, UNSUPPORTED = -1, -3, -4, -6, -7, -8
INTS = [-(2 ** 63), -(2 ** 31) - 1, -2, -1, 0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 64, 255, 256, 4096, 32000, 32001, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 40, 2 ** 62]


def fwd(*a):
    L = _lib.lib()
    rc = L.fql_kd_kl_fwd(*a, None)
    return rc, L.fq_last_error().decode()


def bwd(*a):
    L = _lib.lib()
    rc = L.fql_kd_kl_bwd(*a, None)
    return rc, L.fq_last_error().decode()


# ---- header and binding --------------------------------------------------------------------------------------------------------------------

def test_loss_header_names_equal_loss_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "llmqat_fakequant_loss.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fql_[a-z0-9_]+)\s*\(", src))
    assert declared == set(_lib.LOSS_EXPORTS) == {"fql_kd_kl_fwd", "fql_kd_kl_bwd"}
    assert not re.findall(r"\bfq[tsi]?_[a-z0-9_]+\s*\(", src)      # nothing of the four other families is declared (or named with a call) here
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert not set(_lib.LOSS_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.SR_EXPORTS) | set(_lib.INFER_EXPORTS))
    assert L.fq_version() == _lib.ABI_VERSION == 7
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for f in (L.fql_kd_kl_fwd, L.fql_kd_kl_bwd):
        assert f.argtypes == [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp] and f.restype is i32


def test_the_build_lists_the_new_unit_and_headers():
    src = open(os.path.join(ROOT, "llm-qat_amd", "build.py")).read()
    for name in ("fq_kd_loss.hip", "fq_kd_loss.h", "fq_loss_rows.h", "fq_rows.h", "llmqat_fakequant_loss.h"):
        assert f'"{name}"' in src, name


# ---- refusals, in the header's order: every call is valid up to the check it names and wrong in everything behind it -------------------------

FWD_REFUSALS = [
    # (student, teacher, row_stats, row_loss, loss, rows, cols, batch, dtype), code, part of the message
    ((None, None, None, None, None, -1, -1, 0, 9), DTYPE, "unknown dtype"),
    ((None, None, None, None, None, -1, -1, 0, -1), DTYPE, "unknown dtype"),
    ((None, None, None, None, None, -1, -1, 0, F64), DTYPE, "float64"),
    ((None, None, None, None, None, -3, 8, 0, BF16), SHAPE, "negative shape"),
    ((None, None, None, None, None, 3, -8, 0, F16), SHAPE, "negative shape"),
    ((None, None, None, None, None, 0, 8, 0, F32), SHAPE, "empty shape"),
    ((None, None, None, None, None, 3, 0, 0, BF16), SHAPE, "empty shape"),
    ((None, None, None, None, None, 2 ** 62, 2 ** 40, 0, BF16), SHAPE, "overflows"),
    ((None, None, None, None, None, 3, 8, 0, BF16), ARG, "batch=0"),
    ((None, None, None, None, None, 3, 8, -2, F32), ARG, "batch=-2"),
    ((None, T, ST, RL, LO, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, None, ST, RL, LO, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, ST, None, LO, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, ST, RL, None, 3, 8, 1, BF16), NULL, "NULL"),
    ((None, None, None, None, None, 2 ** 40, 32000, 1, F16), NULL, "NULL"),                  # the pointers come before the grid
    ((S, T, None, RL, LO, 2 ** 33, 2048, 1, BF16), UNSUPPORTED, "exceed one launch's grid"),    # row_stats may be NULL
    ((S, T, ST, RL, LO, 2 ** 34, 8, 1, F32), UNSUPPORTED, "exceed one launch's grid"),
]
BWD_REFUSALS = [
    # (student, teacher, row_stats, grad_loss, grad_student, rows, cols, batch, dtype), code, part of the message
    ((None, None, None, None, None, -1, -1, 0, 9), DTYPE, "unknown dtype"),
    ((None, None, None, None, None, -1, -1, 0, F64), DTYPE, "float64"),
    ((None, None, None, None, None, -3, 8, 0, BF16), SHAPE, "negative shape"),
    ((None, None, None, None, None, 0, 8, 0, F32), SHAPE, "empty shape"),
    ((None, None, None, None, None, 3, 0, 0, F16), SHAPE, "empty shape"),
    ((None, None, None, None, None, 2 ** 62, 2 ** 40, 0, BF16), SHAPE, "overflows"),
    ((None, None, None, None, None, 3, 8, 0, BF16), ARG, "batch=0"),
    ((None, T, ST, G, GS, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, None, ST, G, GS, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, None, G, GS, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, ST, None, GS, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, ST, G, None, 3, 8, 1, BF16), NULL, "NULL"),
    ((S, T, ST, G, S, 3, 8, 1, BF16), ARG, "in-place"),
    ((S, T, ST, G, T, 2 ** 34, 8, 1, F32), ARG, "in-place"),                                    # the aliasing comes before the grid
    ((S, T, ST, G, GS, 2 ** 34, 8, 1, F32), UNSUPPORTED, "exceed one launch's grid"),
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


def test_every_served_dtype_passes_the_first_checks():
    for dtype in (F32, BF16, F16):
        assert fwd(None, None, None, None, None, 3, 32001, 1, dtype)[0] == NULL
        assert bwd(None, None, None, None, None, 3, 32001, 1, dtype)[0] == NULL


def test_fuzz_never_reaches_a_launch():
    rng = random.Random(22)
    L = _lib.lib()
    seen = set()
    clamp = lambda v: max(-(2 ** 31), min(2 ** 31 - 1, v))      # noqa: E731
    for f in (L.fql_kd_kl_fwd, L.fql_kd_kl_bwd):
        for _ in range(400):
            rows, cols, batch = rng.choice(INTS), rng.choice(INTS), rng.choice(INTS)
            rc = f(None, None, None, None, None, rows, cols, batch, clamp(rng.choice(INTS)), None)
            assert rc in (DTYPE, SHAPE, ARG, NULL), (rc, rows, cols, batch)
            assert L.fq_last_error() != b""
            seen.add(rc)
        for _ in range(400):       # the same hostile sizes behind a valid dtype, so that the shape and batch checks are the ones that answer
            rows, cols, batch = rng.choice(INTS), rng.choice(INTS), rng.choice(INTS)
            rc = f(None, None, None, None, None, rows, cols, batch, rng.randrange(3), None)
            assert rc in (SHAPE, ARG, NULL), (rc, rows, cols, batch)
            assert (rc == SHAPE) == (rows <= 0 or cols <= 0 or rows * cols > (2 ** 63 - 1) // 4), (rc, rows, cols)
            assert rc == SHAPE or (rc == ARG) == (batch <= 0), (rc, batch)
            seen.add(rc)
    assert seen == {DTYPE, SHAPE, ARG, NULL}          # never 0, never FQ_ERR_LAUNCH: NULL pointers are never launchable


# ---- the reference helper, on its own ---------------------------------------------------------------------------------------------------------

def test_the_identity_equals_the_kl_div_chain_in_float64():
    for name, (s, t) in R.CASES().items():
        loss64, ds64, *_ = R.ref64(s, t)
        loss, ds = R.formula64(s, t)[:2]
        assert abs(float(loss - loss64)) <= 1e-13 * abs(float(loss64)), name
        assert float((ds - ds64).abs().max()) <= 1e-14, name


def test_the_special_value_table_of_the_formula():
    inf, nan = float("inf"), float("nan")
    base_s, base_t = torch.tensor([[0.5, -1.0, 2.0, 0.25]]), torch.tensor([[1.0, 0.0, -2.0, 0.75]])

    def both(s, t):
        return float(R.formula64(s, t)[0]), float(R.ref64(s, t)[0])
    s, t = base_s.clone(), base_t.clone()
    t[0, 1] = -inf                                           # a teacher -inf: p_t = 0, the term is 0; the chain agrees
    f, c = both(s, t)
    assert math.isfinite(f) and abs(f - c) < 1e-15
    keep = [0, 2, 3]
    assert abs(f - float(R.formula64(s[:, keep], t[:, keep])[0])) > 1e-3      # (the student's entry still counts in lse_s)
    s[0, 2] = -inf                                           # a student -inf where p_t > 0: +inf, as the chain
    assert both(s, t) == (inf, inf)
    s, t = base_s.clone(), base_t.clone()
    s[0, 1] = t[0, 1] = -inf                                 # both -inf at an element: term 0; the chain gives NaN (the documented deviation)
    f, c = both(s, t)
    assert abs(f - float(R.formula64(s[:, keep], t[:, keep])[0])) < 1e-15 and math.isnan(c)
    for which in (0, 1):                                     # a NaN anywhere: NaN
        s, t = base_s.clone(), base_t.clone()
        (s, t)[which][0, 3] = nan
        f, c = both(s, t)
        assert math.isnan(f) and math.isnan(c)
        assert torch.isnan(R.formula64(s, t)[1]).all()
    s, t = base_s.clone(), torch.full((1, 4), -inf)          # a row that is all -inf: NaN, as the chain
    f, c = both(s, t)
    assert math.isnan(f) and math.isnan(c)
    f, c = both(torch.full((1, 4), -inf), base_t)
    assert math.isnan(f) and math.isnan(c)
    s = torch.tensor([[0.0, -2000.0]])                       # p_t underflows: the term is 0 although s is finite and far
    assert both(s, torch.tensor([[0.0, -3000.0]]))[0] == 0.0


def test_the_caps_are_the_size_of_an_eager_chains_error():
    """The caps are 4 x the chain's measures on the MI355X (tests/test_gpu_kd_loss.py checks that the chain sits within CAP / 4 there).
    Here the chain runs on ATen's CPU kernels, which sum in another order (and in one that changes with the thread count): its measures
    are of the caps' order of magnitude and no smaller than the MI355X's, so the caps are no looser than a chain's own error."""
    assert R.LOSS_CAP == 4 * R.EAGER_E_LOSS and R.GRAD_CAP == 4 * R.EAGER_C_GRAD
    m = R.eager_measures("cpu")
    assert set(m) == set(R.CASES()) and len(m) == 8
    worst_loss, worst_grad = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print({k: (round(a, 3), round(b, 2)) for k, (a, b) in m.items()})
    assert R.LOSS_CAP / 16 < worst_loss < 16 * R.LOSS_CAP and R.GRAD_CAP / 16 < worst_grad < 16 * R.GRAD_CAP, (worst_loss, worst_grad)
    assert all(a > 0 and b > 0 for a, b in m.values())                    # every case tells the chain from float64


def test_the_measures_see_an_error_of_their_size():
    s, t = R.CASES()["randn_s3_v4099"]
    ref = R.ref64(s, t)
    loss64, ds64 = ref[0], ref[1]
    n = R.e_loss(loss64 * 0, s, t, ref) * R.UNIT / float(loss64)            # = 1 / N
    assert R.e_loss(loss64, s, t, ref) == 0.0 and R.c_grad(ds64, s, t, ref=ref) == 0.0
    assert R.e_loss(loss64 + 100 * R.UNIT / n, s, t, ref) == pytest.approx(100, rel=1e-6) and 100 > R.LOSS_CAP
    wrong = ds64.clone()
    i = int(((ref[4] - ref[5]).abs() / (ref[4] + ref[5]))[1].argmax())
    wrong[1, i] *= 1 + 2.0 ** -10                            # one element, 16384 fp32 ulp off
    assert R.c_grad(wrong, s, t, ref=ref) > R.GRAD_CAP
    assert R.c_grad(ds64.bfloat16(), s, t, torch.bfloat16, ref=ref) == 0.0                    # the output rounding is allowed for ...
    assert R.c_grad(ds64.bfloat16(), s, t, torch.float32, ref=ref) > R.GRAD_CAP               # ... only where the dtype has it
    assert R.c_grad(0.37 * ds64, s, t, g=0.37, ref=ref) < 1e-3


# ---- install(), the package surface --------------------------------------------------------------------------------------------------------

def test_install_replaces_the_method_and_returns_the_old_one(monkeypatch):
    class Trainer:
        def ce_loss(self, size_average, student_logits, teacher_logits):
            return "old"
    old = Trainer.__dict__["ce_loss"]
    seen = []
    monkeypatch.setattr(distill, "kd_kl_loss", lambda s, t: seen.append((s, t)) or "new")
    assert distill.install(Trainer) is old
    assert Trainer.ce_loss is not old and Trainer().ce_loss(True, 1, 2) == "new" and Trainer().ce_loss(False, 1, 2) == "new"
    assert seen == [(1, 2), (1, 2)]                          # size_average is ignored
    Trainer.ce_loss = old
    assert Trainer().ce_loss(True, 1, 2) == "old"

    class Bare:
        pass
    assert distill.install(Bare) is None and Bare().ce_loss(True, 3, 4) == "new"
    with pytest.raises(TypeError, match="class"):
        distill.install(Trainer())


def test_the_public_names_live_in_the_submodule():
    assert llm_qat_amd.distill is distill and distill.__all__ == ["kd_kl_loss", "install"]
    assert "distill" not in llm_qat_amd.__all__ and "kd_kl_loss" not in llm_qat_amd.__all__ and not hasattr(llm_qat_amd, "kd_kl_loss")
    assert llm_qat_amd.__all__[-2:] == ["MXLinear", "convert_to_mx_inference"]
    assert set(ops.kd_counts) == {"fwd_launch", "bwd_launch", "copy_route"}
    assert "fp32" in distill.kd_kl_loss.__doc__ and "autocast" in distill.kd_kl_loss.__doc__
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "install(KDTrainer)" in text and "fp32" in text


# ---- CPU tensors -----------------------------------------------------------------------------------------------------------------------------

def test_cpu_tensors_are_refused_by_default_and_served_within_the_caps_after_the_opt_in():
    from llm_qat_amd import cpu_tensors
    was = cpu_tensors.ENABLED
    try:
        llm_qat_amd.allow_cpu_tensors(False)
        s, t = R.CASES()["randn_s30_v33"]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            distill.kd_kl_loss(s, t)
        llm_qat_amd.allow_cpu_tensors(True)
        before = dict(ops.kd_counts)
        for name in ("randn_s30_v33", "randn_s3_v4099", "ramp_v2049"):
            s, t = R.CASES()[name]
            for dtype in (torch.float32, torch.bfloat16, torch.float16):
                sd, td = s.detach().to(dtype).clone().requires_grad_(True), t.to(dtype)
                ref = R.ref64(sd, td)
                loss = distill.kd_kl_loss(sd, td)
                assert loss.dtype is torch.float32 and loss.dim() == 0
                (0.37 * loss).backward()
                assert sd.grad.dtype is dtype and sd.grad.shape == sd.shape
                el, cg = R.e_loss(loss, sd, td, ref), R.c_grad(sd.grad, sd, td, dtype, 0.37, ref)
                assert el <= R.LOSS_CAP and cg <= R.GRAD_CAP, (name, dtype, el, cg)
        s3 = s.reshape(1, 2, -1)
        assert float(distill.kd_kl_loss(s3, t.reshape(1, 2, -1))) == pytest.approx(2 * float(distill.kd_kl_loss(s, t)), rel=1e-6)      # batchmean
        assert ops.kd_counts == before                       # no launch, no copy: torch ops
    finally:
        llm_qat_amd.allow_cpu_tensors(was)


# ---- the compiled ops' fake implementations ----------------------------------------------------------------------------------------------------

def test_fake_ops_shapes_and_dtypes_on_meta_tensors():
    assert str(compiled.kd_kl_fwd_op._opoverload._schema) == "llmqat_amd::kd_kl_fwd(Tensor student, Tensor teacher) -> (Tensor, Tensor)"
    assert str(compiled.kd_kl_bwd_op._opoverload._schema) == \
        "llmqat_amd::kd_kl_bwd(Tensor student, Tensor teacher, Tensor row_stats, Tensor grad_loss) -> Tensor"
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for shape in ((6, 515), (2, 3, 32001), (2, 2, 2, 33)):
            s = torch.empty(shape, dtype=dtype, device="meta")
            loss, stats = torch.ops.llmqat_amd.kd_kl_fwd(s, s)
            rows = s.numel() // shape[-1]
            assert loss.device.type == "meta" and loss.shape == () and loss.dtype is torch.float32
            assert tuple(stats.shape) == (rows, 2) and stats.dtype is torch.float32
            g = torch.ops.llmqat_amd.kd_kl_bwd(s, s, stats, loss)
            assert tuple(g.shape) == shape and g.dtype is dtype and g.is_contiguous()
    s = torch.empty(4, 8, dtype=torch.float64, device="meta")
    with pytest.raises(TypeError, match="not served"):
        torch.ops.llmqat_amd.kd_kl_fwd(s, s)
    with pytest.raises(ValueError, match="shape mismatch"):
        torch.ops.llmqat_amd.kd_kl_fwd(s.float(), torch.empty(4, 9, device="meta"))


# ---- Python argument refusals (all before any launch; the device check is the last of them, so CPU tensors reach the others) -----------------

def test_python_argument_refusals():
    s, t = torch.zeros(2, 3, 8), torch.zeros(2, 3, 8)
    before = dict(ops.kd_counts)
    for f in (distill.kd_kl_loss, ops.kd_kl_forward):
        with pytest.raises(TypeError, match="mixed dtypes"):
            f(s.bfloat16(), t)
        with pytest.raises(TypeError, match="float64 is not served|torch.float64 is not served"):
            f(s.double(), t.double())
        with pytest.raises(TypeError, match="torch.int32 is not served"):
            f(s.int(), t.int())
        with pytest.raises(ValueError, match="shape mismatch"):
            f(s, t[:, :2])
        with pytest.raises(ValueError, match="at least two dimensions"):
            f(s[0, 0], t[0, 0])
        with pytest.raises(ValueError, match="empty"):
            f(s[:, :0], t[:, :0])
        with pytest.raises(ValueError, match="teacher_logits requires grad"):
            f(s, t.clone().requires_grad_(True))
        with pytest.raises(TypeError, match="expected a torch.Tensor"):
            f(s, None)
    with torch.no_grad():                                    # grad mode off: a teacher that requires grad is no obstacle; the device is
        with pytest.raises(RuntimeError, match="no CPU"):
            ops.kd_kl_forward(s, t.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.kd_kl_backward(s, t, torch.zeros(6, 2), torch.ones(()))
    assert ops.kd_counts == before
