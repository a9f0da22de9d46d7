"""The fused language-model loss (llm_qat_amd.lm_loss, the fqc_ entry points) on the MI355X: error against float64
within the caps of tests/ce_loss_reference.py at every launch shape, the in-kernel shift against the sliced call, ignored rows that are
never read, no valid row, exact values, labels out of range, the upstream gradient, determinism, canaries, a tensor beyond 2^31
elements, the copy route, peak memory, an end-to-end head, hipGraph capture, torch.compile and install()."""
import math
import types

import pytest
import torch

import llm_qat_amd  # noqa: F401
from llm_qat_amd import _lib, lm_loss, ops
from llm_qat_amd.lm_loss import causal_lm_loss, cross_entropy

import ce_loss_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DCODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
INF, NAN = float("inf"), float("nan")
IGN = R.IGNORE


def randn(shape, seed, sigma=3.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * sigma).to(dtype).cuda()


def labels_for(rows, v, seed):
    """labels whose first valid rows name the first, the last and a middle column; every fourth row, from the second, is ignored"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, v, (rows,), generator=g)
    for r, c in zip([r for r in range(rows) if rows == 1 or r % 4 != 1], (0, v - 1, v // 2)):
        y[r] = c
    if rows > 1:
        y[1::4] = IGN
    return y.cuda()


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def run(x, y, shift=False, reduction="mean", g=None):
    """-> loss, grad of the fused path, and (row_lse, row_loss, n_valid) through the ops, so that the side outputs are seen"""
    x = x.detach().requires_grad_(True)
    loss = (causal_lm_loss if shift else cross_entropy)(x, y, reduction=reduction)
    (grad,) = torch.autograd.grad(loss if g is None else g * loss, x)
    _, row_lse, row_loss, n_valid = ops.ce_forward(x.detach(), y, shift, IGN, reduction)
    return loss.detach(), grad, (row_lse, row_loss, n_valid)


def assert_within_caps(x, y, what, g=None, reduction="mean", ref=None):
    loss, grad, (row_lse, row_loss, n_valid) = run(x, y, reduction=reduction, g=g)
    assert loss.dtype is torch.float32 and loss.dim() == 0 and grad.dtype is x.dtype and grad.shape == x.shape
    ref = ref or R.ref64(x, y, reduction)
    valid = ref[6]
    el, cg = R.e_loss(loss, x, y, reduction, ref), R.c_grad(grad, x, y, x.dtype, 1.0 if g is None else g, reduction, ref)
    print(f"{what}: E_loss {el:.3f} (cap {R.LOSS_CAP:.2f})  C_grad {cg:.2f} (cap {R.GRAD_CAP:.1f})")
    assert el <= R.LOSS_CAP and cg <= R.GRAD_CAP, (what, el, cg)
    assert int(n_valid) == int(valid.sum()) and n_valid.dtype is torch.int64
    rel = ((row_lse.double() - ref[2]).abs() / ref[2].abs().clamp_min(1e-300))[valid].max()
    assert float(rel) <= 2.0 ** -21, (what, float(rel))
    assert int(torch.count_nonzero(bits(grad[~valid]))) == 0 and int(torch.count_nonzero(bits(row_loss[~valid]))) == 0, what
    return loss, grad


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 2), (3, 7), (2, 8), (3, 33), (5, 2047), (5, 2048), (5, 2049), (3, 4099), (2, 32000), (3, 32001), (257, 515)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_shape_within_the_caps(shape):
    y = labels_for(shape[0], shape[1], 3000 + shape[1])
    for dtype in DTYPES:
        assert_within_caps(randn(shape, 1000 + shape[1], dtype=dtype), y, f"{shape} {dtype}")


def test_the_eager_chain_sits_within_a_quarter_of_the_caps_here():
    """the caps are 4 x what this measures: they come from the chain the fused path replaces, on this device, and are not vacuous"""
    m = R.eager_measures("cuda")
    worst_loss, worst_grad = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print({k: (round(a, 4), round(b, 2)) for k, (a, b) in m.items()})
    assert worst_loss <= R.LOSS_CAP / 4 and worst_grad <= R.GRAD_CAP / 4, (worst_loss, worst_grad)
    assert worst_loss > R.LOSS_CAP / 16 and worst_grad > R.GRAD_CAP / 16, (worst_loss, worst_grad)


def test_the_case_list_the_caps_were_measured_on():
    for name, (x, y) in R.CASES().items():
        for dtype in DTYPES:
            assert_within_caps(x.to(dtype).cuda(), y.cuda(), f"{name} {dtype}")


# ---- the shift, done in the kernel ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 5, 33), (2, 3, 2049), (3, 4, 515), (1, 1, 8)], ids=lambda s: "x".join(map(str, s)))
def test_the_shift_in_the_kernel_against_the_sliced_call(shape):
    b, t, v = shape
    for dtype in DTYPES:
        for reduction in ("mean", "sum"):
            x = randn(shape, 40 + v, dtype=dtype)
            lab = labels_for(b * t, v, 41 + v).reshape(b, t)
            lab[:, 0] = IGN                                       # the first label is never used
            if t > 1:
                lab[:, 1] = v // 3                                # ... and the second always is
            before = dict(ops.ce_counts)
            loss, grad, (row_lse, row_loss, n_valid) = run(x, lab, shift=True, reduction=reduction)
            assert ops.ce_counts["copy_route"] == before["copy_route"]                          # no copy
            xs, ys = x[:, :-1].contiguous().reshape(-1, v), lab[:, 1:].contiguous().reshape(-1)
            if t == 1:                                            # every row ignored
                assert int(n_valid) == 0 and int(torch.count_nonzero(bits(grad))) == 0 and int(torch.count_nonzero(bits(row_loss))) == 0
                assert math.isnan(float(loss)) if reduction == "mean" else float(loss) == 0.0
                continue
            wloss, wgrad, (wlse, wrow_loss, wn) = run(xs, ys, reduction=reduction)
            assert int(n_valid) == int(wn) == int((ys != IGN).sum())
            assert torch.equal(bits(row_loss.reshape(b, t)[:, :-1]), bits(wrow_loss)) and torch.equal(bits(row_lse.reshape(b, t)[:, :-1]), bits(wlse))
            assert grad.shape == x.shape and torch.equal(bits(grad[:, :-1]), bits(wgrad))
            assert int(torch.count_nonzero(bits(grad[:, -1]))) == 0 and int(torch.count_nonzero(bits(row_loss.reshape(b, t)[:, -1]))) == 0
            # the float64 sum over rows associates differently (the rows sit at other places of the tree): equal, or the adjacent fp32 value
            assert abs(int(loss.view(torch.int32)) - int(wloss.view(torch.int32))) <= 1, (float(loss), float(wloss))
            if reduction == "mean":
                x64 = x.double()
                assert R.e_loss(loss, xs, ys) <= R.LOSS_CAP and float(loss) == pytest.approx(float(R.chain(x64, lab)), rel=1e-5)


# ---- ignored rows are never read --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(6, 33), (5, 2049), (4, 4096)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ignored_rows_full_of_nan_and_inf_touch_nothing(shape):
    rows, v = shape
    for dtype in DTYPES:
        for shift in (False, True):
            y = labels_for(rows, v, 50 + v)
            lab = y.reshape(1, rows) if shift else y
            x = randn((1, rows, v) if shift else shape, 51 + v, dtype=dtype)
            eff = R.effective_labels(lab, shift)
            ignored = (eff == IGN).nonzero().flatten().tolist()
            assert ignored and len(ignored) < rows
            zeros, dirty = x.clone().reshape(rows, v), x.clone().reshape(rows, v)
            for i, r in enumerate(ignored):
                zeros[r] = 0.0
                dirty[r] = (NAN, INF, -INF)[i % 3]
                dirty[r, ::2] = NAN
            a = run(zeros.reshape(x.shape), lab, shift)
            b = run(dirty.reshape(x.shape), lab, shift)
            assert math.isfinite(float(a[0])) and torch.equal(bits(a[0]), bits(b[0])), (shape, dtype, shift)
            assert torch.equal(bits(a[1]), bits(b[1])) and torch.equal(bits(a[2][1]), bits(b[2][1]))
            assert int(torch.count_nonzero(bits(b[1].reshape(rows, v)[ignored]))) == 0


def test_no_valid_row_is_nan_under_mean_and_zero_under_sum():
    for dtype in DTYPES:
        for shape in ((3, 33), (2, 2048)):
            x = randn(shape, 55, dtype=dtype)
            y = torch.full((shape[0],), IGN, dtype=torch.int64, device="cuda")
            for reduction in ("mean", "sum"):
                loss, grad, (_, row_loss, n_valid) = run(x, y, reduction=reduction)
                assert int(n_valid) == 0 and int(torch.count_nonzero(bits(grad))) == 0 and int(torch.count_nonzero(bits(row_loss))) == 0
                assert math.isnan(float(loss)) if reduction == "mean" else float(loss) == 0.0


# ---- exact values -------------------------------------------------------------------------------------------------------------------------------------

def test_a_row_of_neg_inf_but_zero_at_the_label_is_exactly_zero():
    for dtype in DTYPES:
        for shape in ((3, 33), (2, 2049), (2, 4096)):
            x = torch.full(shape, -INF, dtype=dtype, device="cuda")
            y = labels_for(shape[0], shape[1], 57)
            y[y == IGN] = 5
            x[torch.arange(shape[0], device="cuda"), y] = 0.0
            for reduction in ("mean", "sum"):
                loss, grad, (row_lse, row_loss, _) = run(x, y, reduction=reduction)
                assert float(loss) == 0.0 and int(torch.count_nonzero(grad)) == 0 and not torch.isnan(grad).any(), (dtype, shape)
                assert int(torch.count_nonzero(row_loss)) == 0 and int(torch.count_nonzero(row_lse)) == 0


def test_uniform_rows_give_log_v_and_a_neg_inf_label_logit_gives_inf():
    for dtype in DTYPES:
        for shape in ((3, 33), (2, 2049), (2, 32000)):
            x = torch.full(shape, 1.5, dtype=dtype, device="cuda")
            y = labels_for(shape[0], shape[1], 58)
            loss, grad = assert_within_caps(x, y, f"uniform {shape} {dtype}")
            assert float(loss) == pytest.approx(math.log(shape[1]), rel=1e-6)
            x = randn(shape, 59, dtype=dtype)
            x[0, int(y[0])] = -INF
            loss, grad, (_, row_loss, _) = run(x, y)
            assert float(loss) == INF and float(row_loss[0]) == INF and torch.isfinite(row_loss[1:]).all()
            assert torch.isfinite(grad).all() and R.c_grad(grad, x, y, dtype) <= R.GRAD_CAP


def test_a_nan_in_a_valid_row_stays_in_its_row():
    for dtype in DTYPES:
        for shape in ((4, 2049), (3, 515)):
            x = randn(shape, 60, dtype=dtype)
            y = labels_for(shape[0], shape[1], 61)
            x[2, shape[1] - 2] = NAN
            loss, grad, (row_lse, row_loss, _) = run(x, y)
            assert math.isnan(float(loss)) and math.isnan(float(row_loss[2])) and torch.isnan(grad[2]).all()
            clean = x.clone()
            clean[2] = clean[0]
            ref = R.ref64(clean, y)
            keep = torch.tensor([r != 2 for r in range(shape[0])], device="cuda")
            assert torch.isfinite(grad[keep]).all()
            part = tuple(t if t.dim() == 0 else t[keep] for t in ref)
            cg = R.c_grad(grad[keep], x[keep], y[keep], dtype, ref=part, n=int(ref[6].sum()))      # the NaN row counts in n
            assert cg <= R.GRAD_CAP, (dtype, shape, cg)


# ---- labels out of range: compared, never an address ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["cols", -1, -5])
def test_a_label_out_of_range_is_nan_in_its_row_and_touches_no_other(bad):
    for dtype in DTYPES:
        for shape in ((4, 33), (4, 2049), (4, 4096)):
            rows, v = shape
            x = randn(shape, 62 + v, dtype=dtype)
            y = labels_for(rows, v, 63)                        # row 1 is ignored
            good = y.clone()
            y[2] = v if bad == "cols" else bad
            for shift in (False, True):
                xx, yy, gg = (x.reshape(1, rows, v), y.reshape(1, rows), good.reshape(1, rows)) if shift else (x, y, good)
                loss, grad, (row_lse, row_loss, n_valid) = run(xx, yy, shift)
                grad, eff = grad.reshape(rows, v), R.effective_labels(yy, shift)
                r = int((eff == y[2]).nonzero()[0])             # the row that sees the bad label
                eff_good = R.effective_labels(gg, shift)
                assert int(n_valid) == int((eff != IGN).sum())                       # the row counts as valid
                assert math.isnan(float(loss)) and math.isnan(float(row_loss[r])) and torch.isnan(grad[r]).all(), (bad, dtype, shape, shift)
                others = torch.tensor([i != r for i in range(rows)], device="cuda")
                assert torch.isfinite(grad[others]).all() and torch.isfinite(row_loss[others]).all()
                ref = R.ref64(x, eff_good)                      # the same n: the bad row counted
                part = tuple(t if t.dim() == 0 else t[others] for t in ref)
                cg = R.c_grad(grad[others], x[others], eff_good[others], dtype, ref=part, n=int(ref[6].sum()))
                assert cg <= R.GRAD_CAP, (bad, dtype, shape, shift, cg)


# ---- the upstream gradient, the reduction, launches, determinism -----------------------------------------------------------------------------------------

def test_upstream_gradient_sum_no_grad_and_logits_without_grad():
    for dtype in DTYPES:
        x, y = randn((10, 2049), 31, dtype=dtype), labels_for(10, 2049, 32)
        assert_within_caps(x, y, f"g = 0.37 {dtype}", g=0.37)
        assert_within_caps(x, y, f"sum {dtype}", reduction="sum")
        assert_within_caps(x, y, f"sum, g = -2.5 {dtype}", g=-2.5, reduction="sum")
        xg = x.clone().requires_grad_(True)
        (0.0 * cross_entropy(xg, y)).backward()
        assert int(torch.count_nonzero(xg.grad)) == 0
        before = dict(ops.ce_counts)
        with torch.no_grad():
            loss = cross_entropy(xg, y)
        assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.ce_counts["bwd_launch"] == before["bwd_launch"]
        assert not loss.requires_grad and loss.untyped_storage().nbytes() == 4 * (2 + 10 + 1)      # n_valid, row_loss, loss: no stats buffer
        assert cross_entropy(xg, y).untyped_storage().nbytes() == 4 * (2 + 2 * 10 + 1)
        loss = causal_lm_loss(x.reshape(2, 5, 2049), y.reshape(2, 5))                              # logits that do not require grad
        assert not loss.requires_grad and loss.grad_fn is None and loss.untyped_storage().nbytes() == 4 * (2 + 10 + 1)
        assert ops.ce_counts["bwd_launch"] == before["bwd_launch"]


def test_two_runs_are_bit_identical():
    for dtype in DTYPES:
        for shape in ((5, 2049), (3, 32001), (257, 515)):
            x, y = randn(shape, 11, dtype=dtype), labels_for(shape[0], shape[1], 12)
            a, b = run(x, y), run(x, y)
            for p, q in zip((a[0], a[1]) + a[2], (b[0], b[1]) + b[2]):
                assert torch.equal(bits(p), bits(q)), (shape, dtype)


# ---- canaries: the entry points write their outputs and nothing else --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 33), (3, 32001), (5, 2112)], ids=lambda s: f"{s[0]}x{s[1]}")      # element path twice, 16-byte path
def test_canaries_around_every_output(shape):
    rows, cols = shape
    L = _lib.lib()
    for dtype in DTYPES:
        for shift, seq in ((0, rows), (1, rows), (1, 1)):
            x, y = randn(shape, 41, dtype=dtype), labels_for(rows, cols, 42)
            x0, y0 = x.clone(), y.clone()
            sizes = {"grad": x.numel() * x.element_size(), "lse": rows * 4, "row_loss": rows * 4, "loss": 4, "n": 8}
            bufs = {k: torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
            ptr = {k: b.data_ptr() + 64 for k, b in bufs.items()}
            g = torch.full((1,), 0.5, device="cuda")
            args = (rows, cols, seq, shift, IGN, _lib.CE_MEAN, DCODE[dtype])
            _lib.check(ops._launch(x, L.fqc_ce_fwd, x.data_ptr(), y.data_ptr(), ptr["lse"], ptr["row_loss"], ptr["loss"], ptr["n"], *args), "fqc_ce_fwd")
            _lib.check(ops._launch(x, L.fqc_ce_bwd, x.data_ptr(), y.data_ptr(), ptr["lse"], ptr["n"], g.data_ptr(), ptr["grad"], *args), "fqc_ce_bwd")
            torch.cuda.synchronize()
            for k, b in bufs.items():
                assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all(), (k, dtype, shift, seq)
            assert torch.equal(x, x0) and torch.equal(y, y0) and float(g) == 0.5
            eff = R.effective_labels(y.reshape(rows // seq, seq), bool(shift))
            n = int(bufs["n"][64:-64].view(torch.int64)[0])
            grad = bufs["grad"][64:-64].view(dtype).reshape(shape)
            row_loss = bufs["row_loss"][64:-64].view(torch.float32)
            loss = bufs["loss"][64:-64].view(torch.float32)[0]
            assert n == int((eff != IGN).sum())
            if n == 0:                                          # seq_len 1 under the shift: every row is the last of its sequence
                assert math.isnan(float(loss)) and int(torch.count_nonzero(bits(grad))) == 0
                continue
            ref = R.ref64(x, eff)
            assert R.e_loss(loss, x, eff, ref=ref) <= R.LOSS_CAP and R.c_grad(grad, x, eff, dtype, 0.5, ref=ref) <= R.GRAD_CAP
            assert float(row_loss.double().sum() / n) == pytest.approx(float(loss), rel=2.0 ** -22)


# ---- more than 2^31 elements ------------------------------------------------------------------------------------------------------------------------

def test_a_tensor_beyond_2_31_elements():
    rows, cols = 65537, 32768
    if torch.cuda.mem_get_info()[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    x = torch.randn(rows, cols, device="cuda", dtype=torch.bfloat16).mul_(3)
    y = torch.randint(0, cols, (rows,), device="cuda")
    y[1], y[rows - 2] = IGN, IGN
    y[0], y[rows - 1] = cols - 1, 0
    assert x.numel() > 2 ** 31
    loss, row_lse, row_loss, n_valid = ops.ce_forward(x, y)
    grad = ops.ce_backward(x, y, row_lse, n_valid, torch.ones((), device="cuda"))
    assert math.isfinite(float(loss)) and float(loss) > 0 and int(n_valid) == rows - 2
    for sl in (slice(0, 4), slice(rows - 4, rows)):
        xs, ys = x[sl], y[sl]
        ref = R.ref64(xs, ys)
        valid = ref[6]
        assert float(((row_lse[sl].double() - ref[2]).abs() / ref[2].abs())[valid].max()) <= 2.0 ** -21
        assert float(((row_loss[sl].double() - (ref[2] - ref[3])).abs() / (ref[2].abs() + ref[3].abs()))[valid].max()) <= 2.0 ** -21
        assert R.c_grad(grad[sl], xs, ys, torch.bfloat16, 3 / (rows - 2), ref=ref) <= R.GRAD_CAP      # d64 of the slice is for its own n = 3
        assert int(torch.count_nonzero(bits(grad[sl][~valid]))) == 0
    del grad


# ---- non-contiguous inputs --------------------------------------------------------------------------------------------------------------------------

def test_views_take_the_copy_route_and_give_the_contiguous_result():
    for dtype in DTYPES:
        full = randn((2, 9, 515), 51, dtype=dtype)
        lab = labels_for(18, 515, 52).reshape(2, 9)
        views = [(full[..., :-1, :], lab[..., 1:], 2),                                                        # the reference's two slices
                 (randn((2, 515, 8), 53, dtype=dtype).transpose(1, 2), lab[:, :8].contiguous(), 1),
                 (full[..., :-1, :], lab[..., 1:].contiguous(), 1)]
        for xv, yv, n_copies in views:
            assert not xv.is_contiguous()
            want = run(xv.contiguous(), yv.contiguous())
            before = dict(ops.ce_counts)
            xg = xv.detach().requires_grad_(True)
            loss = cross_entropy(xg, yv)
            (grad,) = torch.autograd.grad(loss, xg)
            assert ops.ce_counts["copy_route"] == before["copy_route"] + n_copies
            assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.ce_counts["bwd_launch"] == before["bwd_launch"] + 1
            assert torch.equal(loss, want[0]) and grad.shape == xv.shape and torch.equal(bits(grad), bits(want[1]))


# ---- memory -----------------------------------------------------------------------------------------------------------------------------------------

def _peak_over_baseline(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_peak_memory_is_the_gradient_and_the_side_outputs():
    x = randn((2, 64, 4096), 61, dtype=torch.bfloat16).requires_grad_(True)
    lab = labels_for(128, 4096, 62).reshape(2, 64)
    nbytes = x.numel() * x.element_size()

    def fused():
        x.grad = None
        causal_lm_loss(x, lab).backward()

    def eager():
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = R.chain(x, lab)
        loss.backward()
    fused(), eager()                                   # warm-up: code objects, the autograd engine's own buffers
    x.grad = None
    fused_peak = _peak_over_baseline(fused)
    x.grad = None
    eager_peak = _peak_over_baseline(eager)
    print(f"peak over baseline: fused {fused_peak} bytes, eager {eager_peak} bytes, logits {nbytes} bytes")
    assert eager_peak > 4 * nbytes                     # the yardstick: the shift copy 1 x, the fp32 cast 2 x, the log-softmax 2 x, times 63 / 64
    assert fused_peak <= nbytes + 64 * 1024            # the gradient, 8 * rows + 12 bytes of side outputs, allocator rounding


# ---- end to end: a head under autocast ---------------------------------------------------------------------------------------------------------------

def test_a_linear_head_under_autocast_trains_as_with_the_eager_chain():
    torch.manual_seed(5)
    head = torch.nn.Linear(64, 515).cuda()
    h = randn((2, 16, 64), 71, 1.0)
    lab = labels_for(32, 515, 72).reshape(2, 16)

    def grads(loss_fn, dtype=None):
        hh = h.clone().to(dtype or h.dtype).requires_grad_(True)
        m = head if dtype is None else torch.nn.Linear(64, 515).cuda().to(dtype)
        if dtype is not None:
            m.load_state_dict({k: v.to(dtype) for k, v in head.state_dict().items()})
        m.zero_grad()
        if dtype is None:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = m(hh)
                loss = loss_fn(logits, lab)
        else:
            logits = m(hh)
            loss = loss_fn(logits, lab)
        loss.backward()
        return loss.detach(), logits.detach(), m.weight.grad.double(), hh.grad.double()
    before = dict(ops.ce_counts)
    f_loss, f_logits, f_w, f_h = grads(causal_lm_loss)
    assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.ce_counts["bwd_launch"] == before["bwd_launch"] + 1
    assert ops.ce_counts["copy_route"] == before["copy_route"]
    e_loss, e_logits, e_w, e_h = grads(R.chain)
    _, _, w64, h64 = grads(R.chain, torch.float64)
    assert f_logits.dtype is torch.bfloat16 and torch.equal(f_logits, e_logits) and f_loss.dtype is torch.float32
    xs, ys = f_logits[:, :-1].reshape(-1, 515), lab[:, 1:].reshape(-1)
    el = R.e_loss(f_loss, xs, ys)
    assert el <= R.LOSS_CAP, el
    for name, f, e, r in (("weight", f_w, e_w, w64), ("input", f_h, e_h, h64)):
        ef, ee = float((f - r).abs().max()), float((e - r).abs().max())
        print(f"{name} gradient: max error against float64: fused {ef:.3e}, eager {ee:.3e}; scale {float(r.abs().max()):.3e}")
        assert ef <= 4 * ee, (name, ef, ee)


# ---- hipGraph -----------------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_forward_and_backward_replays_bit_for_bit():
    shape = (2, 8, 2049)
    for dtype in DTYPES:
        x_static = randn(shape, 81, dtype=dtype).requires_grad_(True)
        lab_static = labels_for(16, 2049, 82).reshape(2, 8)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside the capture
            torch.autograd.grad(causal_lm_loss(x_static, lab_static), x_static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = causal_lm_loss(x_static, lab_static)
            (grad,) = torch.autograd.grad(loss, x_static)
        for seed in (83, 85):                              # other logits, other labels, another count of valid rows: all read on the device
            x_new, lab_new = randn(shape, seed, 4.0, dtype), labels_for(16, 2049, seed + 1).reshape(2, 8)
            lab_new[1, seed % 7 + 1] = IGN
            with torch.no_grad():
                x_static.copy_(x_new)
                lab_static.copy_(lab_new)
            graph.replay()
            torch.cuda.synchronize()
            want_loss, want_grad, _ = run(x_new, lab_new, shift=True)
            assert torch.equal(loss.detach(), want_loss) and torch.equal(bits(grad), bits(want_grad)), (dtype, seed)


# ---- torch.compile ------------------------------------------------------------------------------------------------------------------------------------

def test_compiles_to_one_graph_with_the_eager_bits():
    from torch._dynamo.utils import counters

    def f(x, lab):
        return causal_lm_loss(x * 1.0, lab) * 2.0 + cross_entropy(x[:, 0] * 1.0, lab[:, 0], reduction="sum")
    for dtype in (torch.bfloat16, torch.float32):
        torch._dynamo.reset()
        counters.clear()
        x, lab = randn((2, 3, 2049), 91, dtype=dtype), labels_for(6, 2049, 92).reshape(2, 3)
        lab[0, 0] = 7
        xe = x.clone().requires_grad_(True)
        want = f(xe, lab)
        want.backward()
        xc = x.clone().requires_grad_(True)
        before = dict(ops.ce_counts)
        out = torch.compile(f, fullgraph=True, backend="aot_eager")(xc, lab)
        out.backward()
        assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.ce_counts["bwd_launch"] == before["bwd_launch"] + 2
        assert torch.equal(out.detach(), want.detach()) and torch.equal(bits(xc.grad), bits(xe.grad)), dtype
        assert counters["stats"]["unique_graphs"] == 1 and not counters["graph_break"], dict(counters["stats"])


# ---- install() ----------------------------------------------------------------------------------------------------------------------------------------

def test_install_routes_a_model_shaped_forward_through_the_fused_path():
    ns = types.ModuleType("modeling_stand_in")
    ns.CrossEntropyLoss = torch.nn.CrossEntropyLoss

    def forward(logits, labels):                           # the shape of a causal LM's loss lines, looking the class up in its module
        shift_logits = logits[..., :-1, :].contiguous()
        shift_labels = labels[..., 1:].contiguous()
        return ns.CrossEntropyLoss()(shift_logits.view(-1, logits.shape[-1]), shift_labels.view(-1))
    x = randn((2, 4, 515), 95, dtype=torch.bfloat16).requires_grad_(True)
    lab = labels_for(8, 515, 96).reshape(2, 4)
    old = lm_loss.install(ns)
    assert old is torch.nn.CrossEntropyLoss
    before = dict(ops.ce_counts)
    loss = forward(x, lab)
    loss.backward()
    assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.ce_counts["bwd_launch"] == before["bwd_launch"] + 1
    assert ops.ce_counts["copy_route"] == before["copy_route"]            # the model's own shift copy is contiguous already
    xs, ys = x.detach()[:, :-1].reshape(-1, 515), lab[:, 1:].reshape(-1)
    assert loss.dtype is torch.float32 and R.e_loss(loss, xs, ys) <= R.LOSS_CAP
    assert R.c_grad(x.grad[:, :-1].reshape(-1, 515), xs, ys, torch.bfloat16) <= R.GRAD_CAP and int(torch.count_nonzero(x.grad[:, -1])) == 0
    fused = causal_lm_loss(x.detach(), lab)                               # the one-line edit gives the same rows without the copy
    assert abs(int(fused.view(torch.int32)) - int(loss.detach().view(torch.int32))) <= 1
    ns.CrossEntropyLoss = old                                             # the undo: ATen's chain again, and no further launch of ours
    assert float(forward(x.detach().float(), lab)) == pytest.approx(float(loss), rel=1e-5)
    assert ops.ce_counts["fwd_launch"] == before["fwd_launch"] + 2
