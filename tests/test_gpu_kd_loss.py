"""The fused distillation loss (llm_qat_amd.distill.kd_kl_loss, the fql_ entry points) on the MI355X: error against
float64 within the caps of tests/kd_loss_reference.py at every launch shape and row pattern, the exact zero of kd(s, s), determinism,
batchmean, the upstream gradient, canaries, a tensor beyond 2^31 elements, the copy route, peak memory, an end-to-end head, hipGraph
capture, torch.compile and install()."""
import math

import pytest
import torch

import llm_qat_amd  # noqa: F401
from llm_qat_amd import _lib, distill, ops
from llm_qat_amd.distill import kd_kl_loss

import kd_loss_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DCODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
INF, NAN = float("inf"), float("nan")


def randn(shape, seed, sigma=3.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * sigma).to(dtype).cuda()


def run(s, t, g=None):
    """-> loss, grad, row_stats of the fused path (through the ops, so that the stats are seen)"""
    s = s.detach().requires_grad_(True)
    loss = kd_kl_loss(s, t)
    (grad,) = torch.autograd.grad(loss if g is None else g * loss, s)
    return loss.detach(), grad, ops.kd_kl_forward(s.detach(), t)[1]


def assert_within_caps(s, t, what, g=None, ref=None):
    loss, grad, stats = run(s, t, g)
    assert loss.dtype is torch.float32 and loss.dim() == 0 and grad.dtype is s.dtype and grad.shape == s.shape
    ref = ref or R.ref64(s, t)
    el, cg = R.e_loss(loss, s, t, ref), R.c_grad(grad, s, t, s.dtype, 1.0 if g is None else g, ref)
    print(f"{what}: E_loss {el:.3f} (cap {R.LOSS_CAP:.2f})  C_grad {cg:.2f} (cap {R.GRAD_CAP:.1f})")
    assert el <= R.LOSS_CAP and cg <= R.GRAD_CAP, (what, el, cg)
    want = torch.stack([ref[2].reshape(-1), ref[3].reshape(-1)], dim=1)
    rel = ((stats.double() - want).abs() / want.abs().clamp_min(1e-300)).max()
    assert stats.shape == want.shape and float(rel) <= 2.0 ** -21, (what, float(rel))
    return loss, grad


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 2), (3, 7), (2, 8), (3, 33), (5, 2047), (5, 2048), (5, 2049), (3, 4099), (2, 32000), (3, 32001), (257, 515)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_shape_within_the_caps(shape):
    for dtype in DTYPES:
        s, t = randn(shape, 1000 + shape[1], dtype=dtype), randn(shape, 2000 + shape[1], dtype=dtype)
        assert_within_caps(s, t, f"{shape} {dtype}")


def test_the_eager_chain_sits_within_a_quarter_of_the_caps_here():
    """the caps are 4 x what this measures: they come from the chain the fused path replaces, on this device, and are not vacuous"""
    m = R.eager_measures("cuda")
    worst_loss, worst_grad = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print({k: (round(a, 4), round(b, 2)) for k, (a, b) in m.items()})
    assert worst_loss <= R.LOSS_CAP / 4 and worst_grad <= R.GRAD_CAP / 4, (worst_loss, worst_grad)
    assert worst_loss > R.LOSS_CAP / 16 and worst_grad > R.GRAD_CAP / 16, (worst_loss, worst_grad)


def test_the_case_list_the_caps_were_measured_on():
    for name, (s, t) in R.CASES().items():
        for dtype in DTYPES:
            assert_within_caps(s.to(dtype).cuda(), t.to(dtype).cuda(), f"{name} {dtype}")


# ---- row patterns ---------------------------------------------------------------------------------------------------------------------------------

def _pattern(name, shape, seed):
    """-> s, t (fp32, CPU) and what the pattern expects: "caps" | "formula" (the chain gives NaN) | "inf" | "nan" """
    rows, v = shape
    s, t = randn(shape, seed).cpu(), randn(shape, seed + 1).cpu()
    ramp = torch.linspace(-6.0, 6.0, v).repeat(rows, 1)
    kind = "caps"
    if name == "max_first":
        s[:, 0], t[:, 0] = 15.0, 14.0
    elif name == "max_last":
        s[:, -1], t[:, -1] = 15.0, 14.0
    elif name == "ascending":                       # every vector rescales
        s, t = ramp.clone(), 0.5 * ramp
    elif name == "descending":
        s, t = -ramp, -0.5 * ramp
    elif name == "constant":
        s, t = torch.full(shape, 1.5), torch.full(shape, -2.0)
    elif name == "one_logit_80_above":
        s[:, v // 3] += 80.0
        t[:, v // 2] += 80.0
    elif name == "p_t_underflows":
        s, t = 3.0 * ramp, -10.0 * ramp - 60.0      # t spans [-120, 0]: p_t underflows in fp32 below about -87
    elif name == "teacher_neg_inf":
        t[:, 1::3] = -INF
        t[0, : v // 2] = -INF
    elif name == "both_neg_inf":
        s[1, 5] = t[1, 5] = -INF
        s[0, v - 1] = t[0, v - 1] = -INF
        kind = "formula"
    elif name == "student_neg_inf":
        s[1, v // 2] = -INF
        kind = "inf"
    elif name == "nan_in_one_row":
        (s if seed % 2 else t)[1, v - 2] = NAN
        kind = "nan"
    return s, t, kind


PATTERNS = ["max_first", "max_last", "ascending", "descending", "constant", "one_logit_80_above", "p_t_underflows", "teacher_neg_inf",
            "both_neg_inf", "student_neg_inf", "nan_in_one_row"]


@pytest.mark.parametrize("shape", [(4, 2049), (2, 4099)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", PATTERNS)
def test_row_patterns(name, shape):
    for i, dtype in enumerate(DTYPES):
        s, t, kind = _pattern(name, shape, 300 + i)
        s, t = s.to(dtype).cuda(), t.to(dtype).cuda()
        what = f"{name} {shape} {dtype}"
        if kind == "caps":
            assert_within_caps(s, t, what)
        elif kind == "formula":
            assert math.isnan(float(R.ref64(s, t)[0]))                     # the documented deviation: the chain gives NaN, the term is 0
            assert_within_caps(s, t, what, ref=R.formula64(s, t))
        elif kind == "inf":
            loss, grad, stats = run(s, t)
            ref = R.formula64(s, t)
            assert float(loss) == INF and float(ref[0]) == INF, what
            assert torch.isfinite(grad).all() and R.c_grad(grad, s, t, dtype, ref=ref) <= R.GRAD_CAP, what
        else:
            loss, grad, stats = run(s, t)
            assert math.isnan(float(loss)), what
            assert torch.isnan(grad[1]).all() and torch.isnan(stats[1]).any(), what
            clean = s.clone(), t.clone()
            clean[0][1], clean[1][1] = clean[0][0], clean[1][0]
            ref = R.ref64(*clean)
            keep = [r for r in range(shape[0]) if r != 1]
            part = tuple(x if x.dim() == 0 else x[keep] for x in ref)
            assert torch.isfinite(grad[keep]).all() and R.c_grad(grad[keep], s, t, dtype, ref=part) <= R.GRAD_CAP, what


# ---- symmetry, determinism, batchmean ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 4099), (2, 32001)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_student_that_equals_the_teacher_has_zero_loss_and_zero_gradient(shape):
    for dtype in DTYPES:
        for sigma in (1.0, 8.0):
            s = randn(shape, 7, sigma, dtype).requires_grad_(True)
            loss = kd_kl_loss(s, s.detach())
            loss.backward()
            assert float(loss) == 0.0 and int(torch.count_nonzero(s.grad)) == 0, (shape, dtype, sigma, float(loss))
        e_loss, e_grad = R.eager32(s, s.detach())
        print(f"{shape} {dtype}: the eager chain gives loss {float(e_loss):.3e}, {int(torch.count_nonzero(e_grad))} non-zero gradient elements")


def test_two_runs_are_bit_identical():
    for dtype in DTYPES:
        for shape in ((5, 2049), (3, 32001), (257, 515)):
            s, t = randn(shape, 11, dtype=dtype), randn(shape, 12, dtype=dtype)
            a, b = run(s, t), run(s, t)
            for x, y in zip(a, b):
                assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), (shape, dtype)


def test_batchmean_divides_by_the_first_dimension():
    for dtype in DTYPES:
        s, t = randn((2, 3, 515), 21, dtype=dtype), randn((2, 3, 515), 22, dtype=dtype)
        l3, g3, _ = run(s, t)
        l2, g2, _ = run(s.reshape(6, 515), t.reshape(6, 515))
        assert float(l3) == pytest.approx(3 * float(l2), rel=2.0 ** -22)
        assert g3.shape == s.shape and R.c_grad(g3, s, t, dtype) <= R.GRAD_CAP
        s4, t4 = s.reshape(1, 2, 3, 515), t.reshape(1, 2, 3, 515)             # a 4-D input is accepted
        l4, g4, _ = run(s4, t4)
        assert float(l4) == pytest.approx(6 * float(l2), rel=2.0 ** -22) and g4.shape == s4.shape
        assert R.e_loss(l4, s4, t4) <= R.LOSS_CAP


# ---- the upstream gradient ------------------------------------------------------------------------------------------------------------------------

def test_upstream_gradient_no_grad_and_a_student_without_grad():
    for dtype in DTYPES:
        s, t = randn((2, 5, 2049), 31, dtype=dtype), randn((2, 5, 2049), 32, dtype=dtype)
        assert_within_caps(s, t, f"g = 0.37 {dtype}", g=0.37)
        sg = s.clone().requires_grad_(True)
        (0.0 * kd_kl_loss(sg, t)).backward()
        assert int(torch.count_nonzero(sg.grad)) == 0
        before = dict(ops.kd_counts)
        with torch.no_grad():
            loss = kd_kl_loss(sg, t)
        assert ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.kd_counts["bwd_launch"] == before["bwd_launch"]
        assert not loss.requires_grad and loss.untyped_storage().nbytes() == 4 * (10 + 1)      # row_loss and loss: no stats buffer
        assert kd_kl_loss(sg, t).untyped_storage().nbytes() == 4 * (3 * 10 + 1)
        loss = kd_kl_loss(s, t)                                                                  # a student that does not require grad
        assert not loss.requires_grad and loss.grad_fn is None and loss.untyped_storage().nbytes() == 4 * (10 + 1)
        assert ops.kd_counts["bwd_launch"] == before["bwd_launch"]


# ---- canaries: the entry points write their outputs and nothing else --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 33), (3, 32001), (5, 2112)], ids=lambda s: f"{s[0]}x{s[1]}")      # element path twice, 16-byte path
def test_canaries_around_every_output(shape):
    rows, cols = shape
    L = _lib.lib()
    for dtype in DTYPES:
        s, t = randn(shape, 41, dtype=dtype), randn(shape, 42, dtype=dtype)
        s0, t0 = s.clone(), t.clone()
        sizes = {"grad": s.numel() * s.element_size(), "stats": rows * 8, "row_loss": rows * 4, "loss": 4}
        bufs = {k: torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
        ptr = {k: b.data_ptr() + 64 for k, b in bufs.items()}
        g = torch.full((1,), 0.5, device="cuda")
        _lib.check(ops._launch(s, L.fql_kd_kl_fwd, s.data_ptr(), t.data_ptr(), ptr["stats"], ptr["row_loss"], ptr["loss"], rows, cols, rows,
                               DCODE[dtype]), "fql_kd_kl_fwd")
        _lib.check(ops._launch(s, L.fql_kd_kl_bwd, s.data_ptr(), t.data_ptr(), ptr["stats"], g.data_ptr(), ptr["grad"], rows, cols, rows,
                               DCODE[dtype]), "fql_kd_kl_bwd")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all(), (k, dtype)
        ref = R.ref64(s, t)
        loss = bufs["loss"][64:-64].view(torch.float32)[0]
        grad = bufs["grad"][64:-64].view(dtype).reshape(shape)
        row_loss = bufs["row_loss"][64:-64].view(torch.float32)
        assert R.e_loss(loss, s, t, ref) <= R.LOSS_CAP and R.c_grad(grad, s, t, dtype, 0.5, ref) <= R.GRAD_CAP
        assert float(row_loss.double().sum() / rows) == pytest.approx(float(loss), rel=2.0 ** -22)
        assert torch.equal(s, s0) and torch.equal(t, t0) and float(g) == 0.5


# ---- more than 2^31 elements ------------------------------------------------------------------------------------------------------------------------

def test_a_tensor_beyond_2_31_elements():
    rows, cols = 65537, 32768
    if torch.cuda.mem_get_info()[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    s = torch.randn(rows, cols, device="cuda", dtype=torch.bfloat16).mul_(3)
    t = torch.randn(rows, cols, device="cuda", dtype=torch.bfloat16).mul_(3)
    assert s.numel() > 2 ** 31
    loss, stats, _ = ops.kd_kl_forward(s, t)
    grad = ops.kd_kl_backward(s, t, stats, torch.ones((), device="cuda"))
    assert math.isfinite(float(loss)) and float(loss) > 0
    for sl in (slice(0, 4), slice(rows - 4, rows)):
        ss, ts = s[sl], t[sl]
        ref = R.ref64(ss, ts)
        want = torch.stack([ref[2], ref[3]], dim=1)
        assert float(((stats[sl].double() - want).abs() / want.abs()).max()) <= 2.0 ** -21
        assert R.c_grad(grad[sl], ss, ts, torch.bfloat16, 4 / rows, ref) <= R.GRAD_CAP      # ds64 of the slice is for batch 4
    del grad


# ---- non-contiguous inputs --------------------------------------------------------------------------------------------------------------------------

def test_views_take_the_copy_route_and_give_the_contiguous_result():
    for dtype in DTYPES:
        full_s, full_t = randn((2, 9, 515), 51, dtype=dtype), randn((2, 9, 515), 52, dtype=dtype)
        views = [(full_s[..., :-1, :], full_t[..., :-1, :]),
                 (randn((2, 515, 8), 53, dtype=dtype).transpose(1, 2), randn((2, 515, 8), 54, dtype=dtype).transpose(1, 2)),
                 (full_s[..., :-1, :], full_t[..., :-1, :].contiguous())]
        for n_copies, (sv, tv) in zip((2, 2, 1), views):
            assert not sv.is_contiguous()
            want = run(sv.contiguous(), tv.contiguous())
            before = dict(ops.kd_counts)
            sg = sv.detach().requires_grad_(True)
            loss = kd_kl_loss(sg, tv)
            (grad,) = torch.autograd.grad(loss, sg)
            assert ops.kd_counts["copy_route"] == before["copy_route"] + n_copies
            assert ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.kd_counts["bwd_launch"] == before["bwd_launch"] + 1
            assert torch.equal(loss, want[0]) and grad.shape == sv.shape and torch.equal(grad.view(torch.uint8), want[1].view(torch.uint8))


# ---- memory -----------------------------------------------------------------------------------------------------------------------------------------

def _peak_over_baseline(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_peak_memory_is_the_gradient_and_the_side_outputs():
    s = randn((2, 64, 4096), 61, dtype=torch.bfloat16).requires_grad_(True)
    t = randn((2, 64, 4096), 62, dtype=torch.bfloat16)
    nbytes = s.numel() * s.element_size()

    def fused():
        s.grad = None
        kd_kl_loss(s, t).backward()

    def eager():
        s.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = R.chain(s, t)
        loss.backward()
    fused(), eager()                                   # warm-up: code objects, the autograd engine's own buffers
    s.grad = None
    fused_peak = _peak_over_baseline(fused)
    s.grad = None
    eager_peak = _peak_over_baseline(eager)
    print(f"peak over baseline: fused {fused_peak} bytes, eager {eager_peak} bytes, student {nbytes} bytes")
    assert eager_peak > 4 * nbytes                     # the yardstick: the chain's fp32 temporaries
    assert fused_peak <= nbytes + 64 * 1024            # the gradient, 12 * rows + 4 bytes of side outputs, allocator rounding


# ---- end to end: a head under autocast ---------------------------------------------------------------------------------------------------------------

def test_a_linear_head_under_autocast_trains_as_with_the_eager_chain():
    torch.manual_seed(5)
    head = torch.nn.Linear(64, 515).cuda()
    h = randn((2, 16, 64), 71, 1.0)
    t = randn((2, 16, 515), 72, dtype=torch.bfloat16)

    def grads(loss_fn, dtype=None):
        hh = h.clone().to(dtype or h.dtype).requires_grad_(True)
        m = head if dtype is None else torch.nn.Linear(64, 515).cuda().to(dtype)
        if dtype is not None:
            m.load_state_dict({k: v.to(dtype) for k, v in head.state_dict().items()})
        m.zero_grad()
        if dtype is None:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = m(hh)
                loss = loss_fn(logits, t)
        else:
            logits = m(hh)
            loss = loss_fn(logits, t.to(dtype))
        loss.backward()
        return loss.detach(), logits.detach(), m.weight.grad.double(), hh.grad.double()
    before = dict(ops.kd_counts)
    f_loss, f_logits, f_w, f_h = grads(kd_kl_loss)
    assert ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.kd_counts["bwd_launch"] == before["bwd_launch"] + 1
    e_loss, e_logits, e_w, e_h = grads(R.chain)
    _, _, w64, h64 = grads(R.chain, torch.float64)
    assert f_logits.dtype is torch.bfloat16 and torch.equal(f_logits, e_logits) and f_loss.dtype is torch.float32
    el = R.e_loss(f_loss, f_logits, t)
    assert el <= R.LOSS_CAP, el
    for name, f, e, r in (("weight", f_w, e_w, w64), ("input", f_h, e_h, h64)):
        ef, ee = float((f - r).abs().max()), float((e - r).abs().max())
        print(f"{name} gradient: max error against float64: fused {ef:.3e}, eager {ee:.3e}; scale {float(r.abs().max()):.3e}")
        assert ef <= 4 * ee, (name, ef, ee)


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_forward_and_backward_replays_bit_for_bit():
    shape = (2, 8, 2049)
    for dtype in DTYPES:
        s_static = randn(shape, 81, dtype=dtype).requires_grad_(True)
        t_static = randn(shape, 82, dtype=dtype)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside the capture
            torch.autograd.grad(kd_kl_loss(s_static, t_static), s_static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = kd_kl_loss(s_static, t_static)
            (grad,) = torch.autograd.grad(loss, s_static)
        for seed in (83, 85):
            s_new, t_new = randn(shape, seed, 4.0, dtype), randn(shape, seed + 1, 2.0, dtype)
            with torch.no_grad():
                s_static.copy_(s_new)
                t_static.copy_(t_new)
            graph.replay()
            torch.cuda.synchronize()
            want_loss, want_grad, _ = run(s_new, t_new)
            assert torch.equal(loss.detach(), want_loss) and torch.equal(grad.view(torch.uint8), want_grad.view(torch.uint8)), (dtype, seed)


# ---- torch.compile ------------------------------------------------------------------------------------------------------------------------------------

def test_compiles_to_one_graph_with_the_eager_bits():
    from torch._dynamo.utils import counters

    def f(s, t):
        return kd_kl_loss(s * 1.0, t) * 2.0
    for dtype in (torch.bfloat16, torch.float32):
        torch._dynamo.reset()
        counters.clear()
        s, t = randn((2, 3, 2049), 91, dtype=dtype), randn((2, 3, 2049), 92, dtype=dtype)
        se = s.clone().requires_grad_(True)
        want = f(se, t)
        want.backward()
        sc = s.clone().requires_grad_(True)
        before = dict(ops.kd_counts)
        out = torch.compile(f, fullgraph=True, backend="aot_eager")(sc, t)
        out.backward()
        assert ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.kd_counts["bwd_launch"] == before["bwd_launch"] + 1
        assert torch.equal(out.detach(), want.detach()) and torch.equal(sc.grad.view(torch.uint8), se.grad.view(torch.uint8)), dtype
        assert counters["stats"]["unique_graphs"] == 1 and not counters["graph_break"], dict(counters["stats"])


# ---- install() ----------------------------------------------------------------------------------------------------------------------------------------

def test_install_routes_a_trainer_through_the_fused_path():
    class Trainer:
        def ce_loss(self, size_average, student_logits, teacher_logits):
            return R.chain(student_logits.float(), teacher_logits.float())
    old = distill.install(Trainer)
    s, t = randn((2, 4, 515), 95, dtype=torch.bfloat16).requires_grad_(True), randn((2, 4, 515), 96, dtype=torch.bfloat16)
    before = dict(ops.kd_counts)
    loss = Trainer().ce_loss(True, s, t)
    loss.backward()
    assert ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.kd_counts["bwd_launch"] == before["bwd_launch"] + 1
    assert R.e_loss(loss, s, t) <= R.LOSS_CAP and R.c_grad(s.grad, s, t, torch.bfloat16) <= R.GRAD_CAP
    Trainer.ce_loss = old
    assert float(Trainer().ce_loss(True, s, t)) == pytest.approx(float(loss), rel=1e-4) and ops.kd_counts["fwd_launch"] == before["fwd_launch"] + 1
