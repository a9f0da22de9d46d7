"""The fused RMSNorm (llm_qat_amd.norm, the fqn_ entry points) on the MI355X: at every launch shape the forward equals
recipe(the kernel's rstd) bit for bit and the errors against float64 stay within the caps of tests/rms_norm_reference.py; the caps against
the eager chain on this device; the reference's own vectors; special values, determinism, canaries, a frozen weight, no_grad, the copy
route, checkpointing, peak memory, hipGraph capture, torch.compile, the class, convert() and install()."""
import os
import types

import numpy as np
import pytest
import torch

import llm_qat_amd  # noqa: F401
from llm_qat_amd import _lib, norm, ops
from llm_qat_amd.norm import rms_norm

import rms_norm_reference as R
import row_ladder_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
MIXED = [(torch.bfloat16, torch.float32), (torch.float16, torch.float32), (torch.float32, torch.bfloat16), (torch.float32, torch.float16)]
DCODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PBITS = {torch.bfloat16: 8, torch.float16: 11}
NAN = float("nan")


def inputs(shape, seed, xdt, wdt, sigma=1.5):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=gen) * sigma).to(xdt).cuda()
    w = (1 + 0.1 * torch.randn(shape[-1], generator=gen)).to(wdt).cuda()
    g = torch.randn(shape, generator=gen).to(wdt).cuda()
    return x, w, g


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def fused(x, w, g, eps=R.EPS):
    y, rstd = ops.rms_norm_forward(x, w, eps)
    dx, dw = ops.rms_norm_backward(g, x, w, rstd)
    return y, rstd, dx, dw


def assert_contract(x, w, g, what, eps=R.EPS):
    y, rstd, dx, dw = fused(x, w, g, eps)
    assert y.dtype is w.dtype and y.shape == x.shape and dx.dtype is x.dtype and dx.shape == x.shape
    assert dw.dtype is w.dtype and dw.shape == w.shape and rstd.dtype is torch.float32 and rstd.shape == (x.numel() // x.shape[-1],)
    ref = R.ref64(x, w, g, eps)
    er, cx, cw = R.e_rstd(rstd, ref), R.c_dx(dx, ref), R.c_dw(dw, g, ref)
    ey = R.e_y(y, w, ref) if y.dtype is torch.float32 else 0.0
    print(f"{what}: E_rstd {er:.3f} (cap {R.RSTD_CAP:.2f})  E_y {ey:.3f} (cap {R.Y_CAP:.2f})  C_dx {cx:.3f} (cap {R.DX_CAP:.2f})  C_dw {cw:.3f} (cap {R.DW_CAP:.2f})")
    assert torch.equal(bits(y), bits(R.recipe(x, w, rstd))), what            # exact, for every dtype, no share left out
    assert er <= R.RSTD_CAP and ey <= R.Y_CAP and cx <= R.DX_CAP and cw <= R.DW_CAP, (what, er, ey, cx, cw)
    return y, rstd, dx, dw


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------------

MOST = 2048            # fqn_rms_norm_bwd_parts at H = 64 for any number of rows from this many up (checked below)
SHAPES = [(1, 1), (1, 8), (3, 7), (2, 8), (5, 33), (4, 256), (3, 2047), (3, 2048), (3, 2049), (2, 4096), (2, 4104), (2, 8200), (2, 11008), (257, 515),
          (MOST, 64), (MOST + 1, 64), (3 * MOST - 1, 64),       # one row per chunk, an uneven last chunk, several rows per chunk
          # several rows per part where a workgroup owns the part (512 parts: the two LDS buffers used in turn, g n summed in registers
          # across rows), and where a row is wider than a sweep (the sums kept in the part's workspace row): 16-byte path > 8192 columns,
          # element path > 4096 for a workgroup and > 1024 for a wave
          (1030, 2048), (1030, 4096), (1027, 8200), (1027, 4099), (4100, 2047)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_shape_equals_the_recipe_and_stays_within_the_caps(shape):
    assert _lib.lib().fqn_rms_norm_bwd_parts(10 ** 9, 64) == MOST
    for dtype in DTYPES:
        assert_contract(*inputs(shape, 1000 + shape[1], dtype, dtype), f"{shape} {dtype}")


@pytest.mark.parametrize("shape", [(5, 33), (3, 2048)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mixed_dtype_pairs(shape):
    for xdt, wdt in MIXED:
        assert_contract(*inputs(shape, 1100 + shape[1], xdt, wdt), f"{shape} x {xdt} w {wdt}")


def test_a_mixed_pair_with_several_wide_rows_per_part():
    """bf16 x under an fp32 weight (autocast over fp32 master weights) at 5120 columns: the element path, two sweeps, three rows per part"""
    shape = (1030, 5120)
    assert _lib.lib().fqn_rms_norm_bwd_parts(*shape) < shape[0] // 2
    for xdt, wdt in MIXED[:1] + MIXED[2:3]:
        assert_contract(*inputs(shape, 1150, xdt, wdt), f"{shape} x {xdt} w {wdt}")


OFFSET_SHAPES = [(5, 256), (3, 2048), (2, 8200), (1027, 4104)]


def offset_by_one(t):
    """the same values in storage that is not 16-byte aligned"""
    n = t.numel()
    out = torch.empty(n + 8, dtype=t.dtype, device="cuda")[1:n + 1].view(t.shape).copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_base_pointer_offset_by_one_element_takes_the_element_path(shape):
    for dtype in DTYPES:
        x, w, g = inputs(shape, 1200 + shape[1], dtype, dtype)
        # (not compared bit for bit with the 16-byte path: the two assign columns to lanes differently, so the sums run in another order)
        assert_contract(offset_by_one(x), w, offset_by_one(g), f"offset {shape} {dtype}")


# ---- the register ladder (tests/row_ladder_cases.py): SHAPES holds the wave path's quarter rung alone -------------------------------------------

LADDER = [(C.rows_of(c), c) for c in C.rms_new_cols(torch.float32)]      # both ends of the wave path's three rungs, the workgroup's full rung filled
LADDER_OFFSET = [(5, 1025)]                                              # the element path's second sweep of a wave, one column in it


@pytest.mark.parametrize("shape", LADDER, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_rung_of_the_ladder_with_a_seeded_row(shape):
    """row 0 holds its largest magnitudes in column 0, in the last column and at the start of the last sweep: a slot past the row that is
    counted, or a last group that is not, moves rstd far beyond its cap (tests/test_row_ladder_cases_cpu.py)"""
    x, w, g = C.rms_inputs(shape[1], shape[0])
    for dtype in DTYPES:
        assert_contract(x.to(dtype).cuda(), w.to(dtype).cuda(), g.to(dtype).cuda(), f"ladder {shape} {dtype}")
    if shape[1] == 1032:
        for xdt, wdt in MIXED:
            assert_contract(x.to(xdt).cuda(), w.to(wdt).cuda(), g.to(wdt).cuda(), f"ladder {shape} x {xdt} w {wdt}")


@pytest.mark.parametrize("shape", LADDER_OFFSET, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_seeded_row_at_a_base_offset_of_one_element(shape):
    x, w, g = C.rms_inputs(shape[1], shape[0])
    for dtype in DTYPES:
        assert_contract(offset_by_one(x.to(dtype).cuda()), w.to(dtype).cuda(), offset_by_one(g.to(dtype).cuda()), f"ladder offset {shape} {dtype}")


# ---- the caps ------------------------------------------------------------------------------------------------------------------------------------

def test_the_eager_chain_sits_within_a_quarter_of_the_caps_here():
    """the caps are 4 x what this measures: they come from the chain the fused path replaces, on this device, and are not vacuous"""
    m = R.eager_measures("cuda")
    worst = [max(v[i] for v in m.values()) for i in range(4)]
    print({k: tuple(round(t, 4) for t in v) for k, v in m.items()})
    for got, cap in zip(worst, (R.RSTD_CAP, R.Y_CAP, R.DX_CAP, R.DW_CAP)):
        assert cap / 16 < got <= cap / 4, (worst, cap)


def test_the_case_list_the_caps_were_measured_on():
    for name, (x, w, g) in R.CASES().items():
        for dtype in DTYPES:
            assert_contract(x.to(dtype).cuda(), w.to(dtype).cuda(), g.to(dtype).cuda(), f"{name} {dtype}")


# ---- the reference's own vectors ---------------------------------------------------------------------------------------------------------------

def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "rms_norm.npz"))

    def load(key, dtype):
        a = z[key]
        return (torch.from_numpy(a.view(np.int16).copy()).view(dtype) if a.dtype == np.uint16 else torch.from_numpy(a.copy())).cuda()
    regular = int(z["regular"])
    for pair in z["pairs"]:
        xd, wd = (DT[p] for p in str(pair).split("_"))
        for h in z["hs"]:
            k = f"{pair}_h{h}_"
            yield str(pair), int(h), regular, float(z[k + "eps"]), load(k + "x", xd), load(k + "w", wd), load(k + "g", wd), load(k + "y", wd)


def test_the_references_vectors():
    """16-bit y: no element more than one unit in the last place from the reference's, and the share that differs at most
    2 RSTD_CAP 2^(p-24): a relative change of rstd by d 2^-24 crosses a rounding boundary of a p-bit significand with probability at most
    d 2^(p-24), and there are two roundings.  fp32 y: both rstd lie within RSTD_CAP of the exact one, and x rstd and its product with w
    round once each.  The special rows agree by NaN position and otherwise bit for bit."""
    differ, total = {torch.bfloat16: 0, torch.float16: 0}, {torch.bfloat16: 0, torch.float16: 0}
    for pair, h, regular, eps, x, w, g, want in golden():
        y, rstd = ops.rms_norm_forward(x, w, eps)
        assert y.dtype is want.dtype
        got, ref = y[:regular], want[:regular]
        if y.dtype is torch.float32:
            rel = ((got.double() - ref.double()).abs() / ref.double().abs().clamp_min(1e-30)).max()
            assert float(rel) <= (2 * R.RSTD_CAP + 2) * R.UNIT, (pair, h, float(rel))
        else:
            ulps = (got.view(torch.int16).int() - ref.view(torch.int16).int()).abs()
            assert int(ulps.max()) <= 1, (pair, h)
            differ[y.dtype] += int((ulps != 0).sum())
            total[y.dtype] += ulps.numel()
        for r in range(regular, x.shape[0]):                                    # zero, NaN, inf, overflow
            assert torch.equal(y[r].isnan(), want[r].isnan()), (pair, h, r)
            assert torch.equal(bits(y[r].nan_to_num(0.0)), bits(want[r].nan_to_num(0.0))), (pair, h, r)
        dx, dw = ops.rms_norm_backward(g, x, w, rstd)
        assert dx[regular + 1].isnan().all() and dw.isnan().all() and torch.isfinite(dx[:regular + 1]).all(), (pair, h)
    for dtype, p in PBITS.items():
        share = differ[dtype] / total[dtype]
        print(f"{dtype}: {differ[dtype]} of {total[dtype]} elements one unit in the last place from the reference's")
        assert total[dtype] >= 500 and share <= 2 * R.RSTD_CAP * 2.0 ** (p - 24), (dtype, share)


# ---- special values, determinism -----------------------------------------------------------------------------------------------------------------

def test_a_nan_row_stays_in_its_row():
    for dtype in DTYPES:
        x, w, g = inputs((6, 2049), 21, dtype, dtype)
        clean = fused(x, w, g)
        bad = x.clone()
        bad[2, 2047] = NAN
        y, rstd, dx, dw = fused(bad, w, g)
        keep = torch.tensor([r != 2 for r in range(6)], device="cuda")
        assert y[2].isnan().all() and dx[2].isnan().all() and dw.isnan().all() and bool(rstd[2].isnan())
        assert torch.equal(bits(y[keep]), bits(clean[0][keep])) and torch.equal(bits(dx[keep]), bits(clean[2][keep])), dtype
        assert torch.equal(bits(rstd[keep]), bits(clean[1][keep]))


def test_zero_rows_inf_and_overflow_follow_the_chain():
    for dtype in DTYPES:
        x, w, g = inputs((5, 515), 22, dtype, dtype)
        x[0] = 0.0
        x[1, 7] = float("inf")
        if dtype is not torch.float16:
            x[2, 9] = 1e20
        y, rstd = ops.rms_norm_forward(x, w, 1e-6)
        assert int(torch.count_nonzero(y[0])) == 0 and float(rstd[0]) == pytest.approx(1e3, rel=1e-6)
        assert float(rstd[1]) == 0.0 and bool(y[1, 7].isnan()) and int(torch.count_nonzero(y[1].nan_to_num(0.0))) == 0
        if dtype is not torch.float16:
            assert float(rstd[2]) == 0.0 and int(torch.count_nonzero(y[2])) == 0
        rec = R.recipe(x, w, rstd)
        assert torch.equal(y.isnan(), rec.isnan()) and torch.equal(bits(y.nan_to_num(0.0)), bits(rec.nan_to_num(0.0)))
        assert torch.equal(y.isnan(), R.chain(x, w).isnan()) and torch.isfinite(y[3:]).all()
        y0, _ = ops.rms_norm_forward(x[:1], w, 0.0)
        assert y0.isnan().all()                                                   # eps = 0 on a zero row: 0 * inf, as the chain


def test_two_runs_are_bit_identical():
    for dtype in DTYPES:
        for shape in ((5, 2049), (2, 11008), (3 * MOST - 1, 64), (257, 515), (1030, 4096), (1027, 8200), (1027, 4099)):
            x, w, g = inputs(shape, 11, dtype, dtype)
            a, b = fused(x, w, g), fused(x, w, g)
            for p, q in zip(a, b):
                assert torch.equal(bits(p), bits(q)), (shape, dtype)


# ---- canaries: the entry points write their outputs and nothing else --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 33), (9, 264), (5, 2112), (2, 8200), (2, 8201), (1030, 4096), (1027, 8200), (1027, 4099)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_canaries_around_every_output(shape):
    rows, cols = shape
    L = _lib.lib()
    for xdt, wdt in [(d, d) for d in DTYPES] + MIXED[:1]:
        x, w, g = inputs(shape, 41, xdt, wdt)
        x0, w0, g0 = x.clone(), w.clone(), g.clone()
        ws_bytes = L.fqn_rms_norm_bwd_workspace_bytes(rows, cols)
        sizes = {"y": x.numel() * w.element_size(), "rstd": rows * 4, "dx": x.numel() * x.element_size(), "dw": cols * w.element_size(), "ws": ws_bytes}
        bufs = {k: torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
        ptr = {k: b.data_ptr() + 64 for k, b in bufs.items()}
        codes = (DCODE[xdt], DCODE[wdt])
        _lib.check(ops._launch(x, L.fqn_rms_norm_fwd, x.data_ptr(), w.data_ptr(), ptr["y"], ptr["rstd"], rows, cols, R.EPS, *codes), "fqn_rms_norm_fwd")
        _lib.check(ops._launch(x, L.fqn_rms_norm_bwd, g.data_ptr(), x.data_ptr(), w.data_ptr(), ptr["rstd"], ptr["dx"], ptr["dw"], ptr["ws"], ws_bytes,
                               rows, cols, *codes), "fqn_rms_norm_bwd")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all(), (k, xdt, wdt)
        assert torch.equal(x, x0) and torch.equal(w, w0) and torch.equal(g, g0)
        want = fused(x, w, g)
        got = (bufs["y"][64:-64].view(wdt).reshape(shape), bufs["rstd"][64:-64].view(torch.float32), bufs["dx"][64:-64].view(xdt).reshape(shape),
               bufs["dw"][64:-64].view(wdt))
        for p, q in zip(got, want):
            assert torch.equal(bits(p), bits(q)), (shape, xdt, wdt)


# ---- what is launched and written ------------------------------------------------------------------------------------------------------------------

class Spy:
    """ops.rms_norm_forward / backward, with the need_* arguments of every call recorded"""

    def __init__(self, monkeypatch):
        self.fwd, self.bwd = [], []
        fwd, bwd = ops.rms_norm_forward, ops.rms_norm_backward

        def forward(x, w, eps=1e-6, need_stats=True):
            self.fwd.append(need_stats)
            out = fwd(x, w, eps, need_stats)
            assert (out[1] is None) == (not need_stats)
            return out

        def backward(g, x, w, rstd, need_dx=True, need_dw=True):
            self.bwd.append((need_dx, need_dw))
            out = bwd(g, x, w, rstd, need_dx, need_dw)
            assert (out[0] is None) == (not need_dx) and (out[1] is None) == (not need_dw)
            return out
        monkeypatch.setattr(ops, "rms_norm_forward", forward)
        monkeypatch.setattr(ops, "rms_norm_backward", backward)


def test_a_frozen_weight_launches_no_dw_stage_and_a_frozen_x_gives_dw_only(monkeypatch):
    spy = Spy(monkeypatch)
    for dtype in DTYPES:
        x, w, g = inputs((7, 2049), 31, dtype, dtype)
        full = fused(x, w, g)
        spy.fwd.clear(), spy.bwd.clear()
        before = dict(ops.norm_counts)
        xg = x.clone().requires_grad_(True)
        rms_norm(xg, w).backward(g)
        assert spy.fwd == [True] and spy.bwd == [(True, False)] and w.grad is None and torch.equal(bits(xg.grad), bits(full[2]))
        wg = w.clone().requires_grad_(True)
        rms_norm(x, wg).backward(g)
        assert spy.bwd[-1] == (False, True) and x.grad is None and torch.equal(bits(wg.grad), bits(full[3]))
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = rms_norm(xg, wg)
        y.backward(g)
        assert spy.bwd[-1] == (True, True) and torch.equal(bits(y), bits(full[0]))
        assert torch.equal(bits(xg.grad), bits(full[2])) and torch.equal(bits(wg.grad), bits(full[3]))
        assert ops.norm_counts["fwd_launch"] == before["fwd_launch"] + 3 and ops.norm_counts["bwd_launch"] == before["bwd_launch"] + 3
    L = _lib.lib()                                       # the C ABI: without dw neither the partial sums nor a workspace
    x, w, g = inputs((7, 2049), 32, torch.bfloat16, torch.bfloat16)
    y, rstd = ops.rms_norm_forward(x, w)
    dx = torch.empty_like(x)
    _lib.check(ops._launch(x, L.fqn_rms_norm_bwd, g.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(), None, None, 0, 7, 2049, 1, 1),
               "fqn_rms_norm_bwd")
    assert torch.equal(bits(dx), bits(ops.rms_norm_backward(g, x, w, rstd)[0]))


def test_no_grad_writes_no_rstd_and_a_transposed_x_takes_the_copy_route(monkeypatch):
    spy = Spy(monkeypatch)
    x, w, g = inputs((4, 33, 515), 33, torch.bfloat16, torch.bfloat16)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    with torch.no_grad():
        y = rms_norm(xg, wg)
    assert spy.fwd == [False] and not y.requires_grad
    y = rms_norm(x, w)                                   # nothing requires grad: no gradient can be asked for
    assert spy.fwd == [False, False] and y.grad_fn is None
    xt = x.transpose(0, 1)
    assert not xt.is_contiguous()
    before = dict(ops.norm_counts)
    xtg = xt.detach().requires_grad_(True)
    yt = rms_norm(xtg, wg)
    yt.backward(g.transpose(0, 1))                       # a non-contiguous g is copied once, too
    assert ops.norm_counts["copy_route"] == before["copy_route"] + 2 and ops.norm_counts["fwd_launch"] == before["fwd_launch"] + 1
    want = fused(xt.contiguous(), w, g.transpose(0, 1).contiguous())
    assert yt.shape == xt.shape and torch.equal(bits(yt), bits(want[0])) and torch.equal(bits(xtg.grad), bits(want[2]))
    assert torch.equal(bits(wg.grad), bits(want[3]))


def test_checkpointing_recomputes_the_first_passs_bits():
    from torch.utils.checkpoint import checkpoint
    for dtype in DTYPES:
        x, w, g = inputs((2, 9, 2048), 34, dtype, dtype)
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        ya = rms_norm(xa, wa)
        ya.backward(g)
        xb, wb = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        before = dict(ops.norm_counts)
        yb = checkpoint(lambda t: rms_norm(t, wb) * 1.0, xb, use_reentrant=False)
        yb.backward(g)
        assert ops.norm_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.norm_counts["bwd_launch"] == before["bwd_launch"] + 1
        assert torch.equal(bits(ya), bits(yb)) and torch.equal(bits(xa.grad), bits(xb.grad)) and torch.equal(bits(wa.grad), bits(wb.grad))


def test_peak_memory_of_the_forward_is_the_output_and_four_bytes_a_row():
    rows, cols = 2048, 4096
    x, w, _ = inputs((rows, cols), 35, torch.bfloat16, torch.bfloat16)
    x.requires_grad_(True)
    rms_norm(x, w)                                       # warm-up: the code object
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = rms_norm(x, w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    want = rows * cols * 2 + 4 * rows
    print(f"peak over the inputs: {peak} bytes; the output and rstd: {want} bytes")
    assert y.grad_fn is not None and want <= peak <= want + 1024       # the allocator rounds a block up to 512 bytes


# ---- hipGraph, torch.compile ---------------------------------------------------------------------------------------------------------------------

def test_a_captured_forward_and_backward_replays_bit_for_bit():
    shape = (2, 8, 2049)
    for dtype in DTYPES:
        x_static, w_static, g_static = inputs(shape, 81, dtype, dtype)
        x_static.requires_grad_(True), w_static.requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside the capture
            torch.autograd.grad(rms_norm(x_static, w_static), (x_static, w_static), g_static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = rms_norm(x_static, w_static)
            dx, dw = torch.autograd.grad(y, (x_static, w_static), g_static)
        for seed in (83, 85):
            x_new, w_new, g_new = inputs(shape, seed, dtype, dtype, 4.0)
            with torch.no_grad():
                x_static.copy_(x_new), w_static.copy_(w_new), g_static.copy_(g_new)
            graph.replay()
            torch.cuda.synchronize()
            want = fused(x_new, w_new, g_new)
            assert torch.equal(bits(y), bits(want[0])) and torch.equal(bits(dx), bits(want[2])) and torch.equal(bits(dw), bits(want[3])), (dtype, seed)


def test_compiles_to_one_graph_with_the_eager_bits():
    from torch._dynamo.utils import counters

    def f(x, w):
        return rms_norm(x * 1.0, w, 1e-5) * 2.0 + norm.rms_norm(x, w.detach())
    for dtype in (torch.bfloat16, torch.float32):
        torch._dynamo.reset()
        counters.clear()
        x, w, g = inputs((2, 3, 2049), 91, dtype, dtype)
        xe, we = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        want = f(xe, we)
        want.backward(g)
        xc, wc = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        before = dict(ops.norm_counts)
        out = torch.compile(f, fullgraph=True, backend="aot_eager")(xc, wc)
        out.backward(g)
        assert ops.norm_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.norm_counts["bwd_launch"] == before["bwd_launch"] + 2
        assert torch.equal(bits(out), bits(want)) and torch.equal(bits(xc.grad), bits(xe.grad)) and torch.equal(bits(wc.grad), bits(we.grad)), dtype
        assert counters["stats"]["unique_graphs"] == 1 and not counters["graph_break"], dict(counters["stats"])


def test_compiled_under_no_grad_writes_no_rstd(monkeypatch):
    spy = Spy(monkeypatch)
    torch._dynamo.reset()
    x, w, _ = inputs((3, 2049), 93, torch.bfloat16, torch.bfloat16)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    f = torch.compile(lambda a, b: rms_norm(a, b) * 1.0, fullgraph=True, backend="aot_eager")
    with torch.no_grad():
        y = f(xg, wg)
    assert spy.fwd == [False] and torch.equal(bits(y), bits(ops.rms_norm_forward(x, w)[0]))
    y = f(x, w)                                          # nothing requires grad
    assert spy.fwd[-1] is False and len(spy.fwd) == 3 and not y.requires_grad     # (the comparison above was the second call)
    y = f(xg, wg)
    assert spy.fwd[-1] is True and y.requires_grad


# ---- the class, convert(), install() ---------------------------------------------------------------------------------------------------------------

def test_the_class_and_a_converted_module_give_the_functions_bits():
    import tiny_llama as TL
    for dtype in DTYPES:
        x, w, g = inputs((3, 5, 256), 95, dtype, dtype)
        want = fused(x, w, g, 1e-5)
        m = norm.RMSNorm(256, eps=1e-5).cuda().to(dtype)
        m.load_state_dict({"weight": w})
        xg = x.clone().requires_grad_(True)
        y = m(xg)
        y.backward(g)
        assert torch.equal(bits(y), bits(want[0])) and torch.equal(bits(xg.grad), bits(want[2])) and torch.equal(bits(m.weight.grad), bits(want[3]))
        holder = torch.nn.Sequential(TL.RMSNorm(256, 1e-5))
        holder[0].variance_epsilon = holder[0].eps       # the harness norm keeps its epsilon under another name
        holder = holder.cuda().to(dtype)
        holder[0].load_state_dict({"weight": w})
        p = holder[0].weight
        assert norm.convert(holder) == 1 and type(holder[0]) is norm.RMSNorm and holder[0].weight is p
        xg = x.clone().requires_grad_(True)
        y = holder(xg)
        y.backward(g)
        assert torch.equal(bits(y), bits(want[0])) and torch.equal(bits(xg.grad), bits(want[2])) and torch.equal(bits(p.grad), bits(want[3]))


def test_install_then_a_model_built_with_the_class_swapped_in_trains(monkeypatch):
    import tiny_llama as TL
    from llm_qat_amd import utils_quant as UQ
    ns = types.ModuleType("modeling_stand_in")
    ns.LlamaRMSNorm = TL.RMSNorm
    assert norm.install(ns) is TL.RMSNorm
    monkeypatch.setattr(TL, "RMSNorm", ns.LlamaRMSNorm)          # the harness model looks its norm class up in its module, as the reference does
    model = TL.load_deterministic(TL.TinyLlama(UQ, w_bits=4, a_bits=8, kv_bits=4).bfloat16()).cuda()
    norms = [m for m in model.modules() if isinstance(m, norm.RMSNorm)]
    assert len(norms) == 2 * TL.TINY["num_hidden_layers"] + 1 and norms[0].variance_epsilon == TL.TINY["rms_norm_eps"]
    ids = TL.deterministic_batch(2, 32).cuda()
    before = dict(ops.norm_counts)
    loss, _ = model(ids, labels=ids)
    loss.backward()
    assert ops.norm_counts["fwd_launch"] == before["fwd_launch"] + len(norms) and ops.norm_counts["bwd_launch"] == before["bwd_launch"] + len(norms)
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
