"""The fused SwiGLU (llm_qat_amd.mlp, the fqa_ entry points) on the MI355X: at every launch shape y, dgate and dup
equal the live eager chain F.silu(gate) * up and its autograd bit for bit, for bf16, fp16 and fp32, no share left out; strided inputs
without a copy, canaries, the reference's special values, a frozen side, no_grad, determinism, what is saved, peak memory, checkpointing,
hipGraph capture, torch.compile, the tiny LLaMA before and after convert() and after install(), and SwiGLUMLP in front of a quantized
down projection."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llm_qat_amd  # noqa: F401
from llm_qat_amd import _lib, mlp, ops
from llm_qat_amd.mlp import swiglu

import swiglu_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DCODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def inputs(shape, seed, dtype):
    """gate at sigma = 3 (both tails of the sigmoid and the zero of its derivative's factor occur), up and dy at sigma = 1"""
    gen = torch.Generator().manual_seed(seed)
    g = (torch.randn(shape, generator=gen) * 3).to(dtype).cuda()
    return g, torch.randn(shape, generator=gen).to(dtype).cuda(), torch.randn(shape, generator=gen).to(dtype).cuda()


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_or_both_nan(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all()) and torch.equal(bits(a.nan_to_num(0.0)), bits(b.nan_to_num(0.0)))


def fused(g, u, dy):
    y = ops.swiglu_forward(g, u)
    dg, du = ops.swiglu_backward(dy, g, u)
    return y, dg, du


def no_zero_sign(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def assert_chain_bits(g, u, dy, what, dg_zero_sign=True):
    """dg_zero_sign=False: dg is compared with every zero taken as +0 (fp16 inputs that reach g <= -88: the sign of a zero dg in the
    remainder behind the last whole 4096-element block of ATen's loop is ATen's own)"""
    before = ops.act_counts["copy_route"]
    y, dg, du = fused(g, u, dy)
    assert ops.act_counts["copy_route"] == before, what
    assert y.dtype is g.dtype and y.shape == g.shape and y.is_contiguous() and dg.shape == du.shape == g.shape
    cy, cdg, cdu = R.chain(g, u, dy)
    for name, got, want in (("y", y, cy), ("dg", dg, cdg), ("du", du, cdu)):
        if name == "dg" and not dg_zero_sign:
            got, want = no_zero_sign(got), no_zero_sign(want)
        assert torch.equal(bits(got), bits(want)), (what, name, int((got != want).sum()), got.numel())
    return y, dg, du


# ---- launch shapes ------------------------------------------------------------------------------------------------------------------------------
# A workgroup owns one tile: 2 vectors a lane on the 16-byte path (4096 16-bit or 2048 fp32 elements), 8 elements a lane on the element
# path (2048).  The walk is flat where every stride equals cols, else row-wise with a tail tile per row.
SHAPES = [(1, 1), (1, 8), (3, 7), (5, 33), (2, 4096), (2, 4104), (3, 11008), (257, 515),
          (1, 4096),        # exactly one 16-bit tile (two fp32 tiles), no tail
          (1, 8200),        # the vector tail: two 16-bit tiles and one vector
          (3, 2049),        # the element path, one element past a tile
          (64, 688)]        # the tiny LLaMA's intermediate size: 16-byte path for 16-bit tensors (1376 bytes a row), fp32 too


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_shape_gives_the_chains_bits(shape):
    for dtype in DTYPES:
        assert_chain_bits(*inputs(shape, 2700 + shape[1], dtype), f"{shape} {dtype}")


@pytest.mark.parametrize("shape", [(5, 256), (2, 4104), (3, 8200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_base_pointer_offset_by_one_element_takes_the_element_path(shape):
    for dtype in DTYPES:
        g, u, dy = inputs(shape, 2800 + shape[1], dtype)
        n = g.numel()
        go = torch.empty(n + 8, dtype=dtype, device="cuda")[1:n + 1].view(shape).copy_(g)
        assert go.data_ptr() % 16 != 0 and go.is_contiguous()
        y, dg, du = assert_chain_bits(go, u, dy, f"offset gate {shape} {dtype}")
        want = fused(g, u, dy)                              # the 16-byte path: the same arithmetic
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip((y, dg, du), want))
        do = torch.empty(n + 8, dtype=dtype, device="cuda")[1:n + 1].view(shape).copy_(dy)
        assert_chain_bits(g, u, do, f"offset dy {shape} {dtype}")


@pytest.mark.parametrize("shape", [(5, 256), (3, 4096), (4, 8200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_odd_row_stride_takes_the_element_path_row_by_row(shape):
    rows, cols = shape
    for dtype in DTYPES:
        g, u, dy = inputs(shape, 2900 + cols, dtype)
        gw = torch.zeros(rows, cols + 1, dtype=dtype, device="cuda")
        gw[:, :cols] = g
        gs = gw[:, :cols]
        assert gs.stride() == (cols + 1, 1) and not gs.is_contiguous()
        y, dg, du = assert_chain_bits(gs, u, dy, f"odd stride {shape} {dtype}")
        want = fused(g, u, dy)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip((y, dg, du), want))


# ---- strided inputs -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 515), (3, 4096), (5, 8200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_halves_of_a_chunk_and_a_row_slice_are_read_where_they_lie(shape):
    """gate, up = t.chunk(2, -1); dy a row slice of a wider tensor: the row-wise walk (element path at 515, 16-byte path with a tail tile per
    row at 8200), no copy, the contiguous call's bits, canaries around every output untouched"""
    rows, cols = shape
    L = _lib.lib()
    for dtype in DTYPES:
        gen = torch.Generator().manual_seed(3000 + cols)
        t = (torch.randn(rows, 2 * cols, generator=gen) * 3).to(dtype).cuda()
        wide = torch.randn(rows, cols + 24, generator=gen).to(dtype).cuda()
        g, u = t.chunk(2, -1)
        dy = wide[:, 8:8 + cols]
        assert not g.is_contiguous() and not u.is_contiguous() and not dy.is_contiguous()
        y, dg, du = assert_chain_bits(g, u, dy, f"chunk {shape} {dtype}")           # (which also asserts that no copy is counted)
        want = fused(g.contiguous(), u.contiguous(), dy.contiguous())
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip((y, dg, du), want))
        t0, wide0 = t.clone(), wide.clone()
        nbytes = rows * cols * t.element_size()
        bufs = {k: torch.full((64 + nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k in ("y", "dg", "du")}
        ptr = {k: b.data_ptr() + 64 for k, b in bufs.items()}
        _lib.check(ops._launch(t, L.fqa_swiglu_fwd, g.data_ptr(), u.data_ptr(), ptr["y"], rows, cols, 2 * cols, 2 * cols, DCODE[dtype]), "fqa_swiglu_fwd")
        _lib.check(ops._launch(t, L.fqa_swiglu_bwd, dy.data_ptr(), g.data_ptr(), u.data_ptr(), ptr["dg"], ptr["du"], rows, cols, cols + 24, 2 * cols,
                               2 * cols, DCODE[dtype]), "fqa_swiglu_bwd")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert (b[:64] == 0xA5).all() and (b[-64:] == 0xA5).all(), (k, dtype)
        assert torch.equal(t, t0) and torch.equal(wide, wide0)
        for k, q in zip(("y", "dg", "du"), want):
            assert torch.equal(bufs[k][64:-64], bits(q)), (k, shape, dtype)


def test_a_three_dimensional_chunk_collapses_to_one_row_stride_and_a_transposed_input_is_copied_once():
    g3, u3, dy3 = inputs((2, 9, 2 * 688), 3100, torch.bfloat16)
    g, u = g3.chunk(2, -1)
    dy = dy3[..., :688]
    before = dict(ops.act_counts)
    y, dg, du = fused(g, u, dy)
    assert ops.act_counts["copy_route"] == before["copy_route"] and y.shape == (2, 9, 688)
    want = fused(g.contiguous(), u.contiguous(), dy.contiguous())
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip((y, dg, du), want))
    gt = g3.transpose(0, 1)                                  # [9, 2, 1376]: the leading dimensions do not collapse
    assert not gt.is_contiguous() and ops.rows_view(gt) is not None
    before = dict(ops.act_counts)
    yt = ops.swiglu_forward(gt, u3.transpose(0, 1).contiguous())
    assert ops.act_counts["copy_route"] == before["copy_route"] + 1 and ops.act_counts["fwd_launch"] == before["fwd_launch"] + 1
    assert yt.shape == gt.shape and torch.equal(bits(yt), bits(ops.swiglu_forward(gt.contiguous(), u3.transpose(0, 1).contiguous())))
    gc = g3.transpose(1, 2)                                  # a last stride that is not 1
    before = dict(ops.act_counts)
    yc = ops.swiglu_forward(gc, gc)
    assert ops.act_counts["copy_route"] == before["copy_route"] + 2 and torch.equal(bits(yc), bits(ops.swiglu_forward(gc.contiguous(), gc.contiguous())))


def test_an_empty_tensor_gives_an_empty_result_without_a_launch():
    g = torch.empty(0, 688, dtype=torch.bfloat16, device="cuda")
    before = dict(ops.act_counts)
    y = ops.swiglu_forward(g, g)
    dg, du = ops.swiglu_backward(g, g, g)
    assert y.shape == dg.shape == du.shape == (0, 688) and ops.act_counts == before
    assert swiglu(g.requires_grad_(True), g).shape == (0, 688) and ops.act_counts == before


# ---- special values, determinism -----------------------------------------------------------------------------------------------------------------

def test_the_special_value_row_of_the_fixture_gives_the_chains_bits_on_the_device():
    z = np.load(os.path.join(ROOT, "tests", "golden", "swiglu.npz"))
    for name, dtype in DT.items():
        def load(key):
            a = z[f"{name}_special_{key}"]
            return (torch.from_numpy(a.view(np.int16).copy()).view(dtype) if a.dtype == np.uint16 else torch.from_numpy(a.copy())).cuda()
        g, u, dy = load("g"), load("u"), load("dy")
        assert g.shape == (1, 40) and bool(g.isnan().any()) and bool(g.isinf().any())
        y, dg, du = fused(g, u, dy)
        cy, cdg, cdu = R.chain(g, u, dy)
        for what, got, want in (("y", y, cy), ("dg", dg, cdg), ("du", du, cdu)):      # NaNs by position, everything else bit for bit
            if name == "f16" and what == "dg":
                # The one place where the chain's bits are not reached: in the remainder behind the last whole block
                # of 4096 elements of ATen's fp16 loop, which is where all 40 elements of this row lie, a dg of -0 is stored as +0 (5 elements:
                # g = -200, -104 against up = 0, 1 and g = -88 against up = 0); in whole blocks ATen keeps -0, as the bf16 and fp32 chains
                # do everywhere.  What holds instead, as the issue provides for: the kernel equals the recipe on the device bit for bit, and
                # no element differs from the chain's as a value
                want_recipe = R.recipe_bwd(dy, g, u)[0]
                assert same_or_both_nan(got, want_recipe), (name, what, got.float().tolist(), want_recipe.float().tolist())
                assert bool(((got == want) | (got.isnan() & want.isnan())).all()), (name, what)
                differ = int((got.view(torch.int16) != want.view(torch.int16)).logical_and(~got.isnan()).sum())
                print(f"fp16 dg: {differ} of 40 elements differ from the chain's in the sign of a zero")
                assert differ <= 5
                continue
            assert same_or_both_nan(got, want), (name, what, got.float().tolist(), want.float().tolist())
        yy = y[0].float()
        assert yy[:1].isnan().all() and yy[4:12].isnan().all()                         # silu(+inf) * 0, silu(-inf), a NaN gate
        assert [str(v) for v in yy[12:15].tolist()] == ["-0.0", "-0.0", "0.0"]       # g = -200: -0 times 0, 1, -1
        # a NaN stays in its element
        g2, u2, dy2 = inputs((3, 515), 3200, dtype)
        clean = fused(g2, u2, dy2)
        g2[1, 7] = float("nan")
        bad = fused(g2, u2, dy2)
        keep = torch.ones(3, 515, dtype=torch.bool, device="cuda")
        keep[1, 7] = False
        for p, q in zip(bad, clean):
            assert bool(p[1, 7].isnan()) and torch.equal(bits(p[keep]), bits(q[keep])), name


def test_two_runs_are_bit_identical():
    for dtype in DTYPES:
        for shape in ((5, 2049), (3, 11008), (257, 515)):
            g, u, dy = inputs(shape, 3300, dtype)
            for p, q in zip(fused(g, u, dy), fused(g, u, dy)):
                assert torch.equal(bits(p), bits(q)), (shape, dtype)


# ---- what is launched, written and saved ------------------------------------------------------------------------------------------------------------

class Spy:
    """ops.swiglu_backward, with the need_* arguments of every call recorded"""

    def __init__(self, monkeypatch):
        self.bwd = []
        bwd = ops.swiglu_backward

        def backward(dy, gate, up, need_dgate=True, need_dup=True, checked=None):
            self.bwd.append((need_dgate, need_dup))
            out = bwd(dy, gate, up, need_dgate, need_dup, checked)
            assert (out[0] is None) == (not need_dgate) and (out[1] is None) == (not need_dup)
            return out
        monkeypatch.setattr(ops, "swiglu_backward", backward)


NODES = ["c++", "python"]


def use_node(monkeypatch, node):
    """mlp.swiglu through the C++ node (the default; it must be there) or through the Python Function"""
    from llm_qat_amd import _act_node
    if node == "python":
        monkeypatch.setattr(_act_node, "load", lambda: None)
    else:
        assert _act_node.load() is not None, _act_node.status()


@pytest.mark.parametrize("node", NODES)
def test_a_frozen_side_is_neither_computed_nor_stored_and_no_grad_saves_nothing(monkeypatch, node):
    use_node(monkeypatch, node)
    spy = Spy(monkeypatch)
    for dtype in DTYPES:
        g, u, dy = inputs((7, 2049), 3400, dtype)
        full = fused(g, u, dy)
        spy.bwd.clear()
        before = dict(ops.act_counts)
        gg = g.clone().requires_grad_(True)
        yg = swiglu(gg, u)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        yg.backward(dy)                                     # up frozen: dgate only
        torch.cuda.synchronize()
        one = gg.grad.numel() * gg.grad.element_size()
        assert one <= torch.cuda.max_memory_allocated() - held < 2 * one      # one gradient was allocated, not two (blocks round up to 512 bytes)
        assert u.grad is None and torch.equal(bits(gg.grad), bits(full[1]))
        ug = u.clone().requires_grad_(True)
        swiglu(g, ug).backward(dy)                          # gate frozen: dup only
        assert g.grad is None and torch.equal(bits(ug.grad), bits(full[2]))
        gg, ug = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        y = swiglu(gg, ug)
        y.backward(dy)
        assert spy.bwd == ([(True, False), (False, True), (True, True)] if node == "python" else [])      # the C++ node does not pass through ops
        assert torch.equal(bits(y), bits(full[0]))
        assert torch.equal(bits(gg.grad), bits(full[1])) and torch.equal(bits(ug.grad), bits(full[2]))
        assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + 3 and ops.act_counts["bwd_launch"] == before["bwd_launch"] + 3
        packed = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
            with torch.no_grad():
                yn = swiglu(gg, ug)
            assert packed == [] and not yn.requires_grad and torch.equal(bits(yn), bits(full[0]))      # no_grad: nothing saved
            yn = swiglu(g, u)                               # nothing requires grad: nothing saved
            assert packed == [] and yn.grad_fn is None
            y = swiglu(gg, ug)
        assert len(packed) == 2 and {t.data_ptr() for t in packed} == {gg.data_ptr(), ug.data_ptr()}       # gate and up, not silu(gate)
    L = _lib.lib()                                          # the C ABI: a NULL output is not written
    g, u, dy = inputs((7, 2049), 3401, torch.bfloat16)
    dg = torch.empty_like(g)
    _lib.check(ops._launch(g, L.fqa_swiglu_bwd, dy.data_ptr(), g.data_ptr(), u.data_ptr(), dg.data_ptr(), None, 7, 2049, 2049, 2049, 2049, 1), "fqa_swiglu_bwd")
    assert torch.equal(bits(dg), bits(ops.swiglu_backward(dy, g, u)[0]))


def test_peak_memory_of_the_forward_is_the_output():
    rows, cols = 2048, 4096
    g, u, _ = inputs((rows, cols), 3500, torch.bfloat16)
    g.requires_grad_(True), u.requires_grad_(True)
    swiglu(g, u)                                            # warm-up: the code object
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = swiglu(g, u)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yc = F.silu(g) * u
    torch.cuda.synchronize()
    eager = torch.cuda.max_memory_allocated() - base
    print(f"peak over the inputs: fused {peak} bytes, eager chain {eager} bytes; the output: {rows * cols * 2} bytes")
    assert y.grad_fn is not None and yc.grad_fn is not None and peak == rows * cols * 2 and eager >= 2 * rows * cols * 2


# ---- checkpointing, hipGraph, torch.compile --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("node", NODES)
def test_checkpointing_recomputes_the_first_passs_bits(monkeypatch, node):
    from torch.utils.checkpoint import checkpoint
    use_node(monkeypatch, node)
    for dtype in DTYPES:
        g, u, dy = inputs((2, 9, 688), 3600, dtype)
        ga, ua = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        ya = swiglu(ga, ua)
        ya.backward(dy)
        gb, ub = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        before = dict(ops.act_counts)
        yb = checkpoint(lambda a, b: swiglu(a, b) * 1.0, gb, ub, use_reentrant=False)
        yb.backward(dy)
        assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.act_counts["bwd_launch"] == before["bwd_launch"] + 1
        assert torch.equal(bits(ya), bits(yb)) and torch.equal(bits(ga.grad), bits(gb.grad)) and torch.equal(bits(ua.grad), bits(ub.grad))


def test_a_captured_forward_and_backward_replays_bit_for_bit():
    shape = (2, 8, 2049)
    for dtype in DTYPES:
        g_static, u_static, dy_static = inputs(shape, 3700, dtype)
        g_static.requires_grad_(True), u_static.requires_grad_(True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside the capture
            torch.autograd.grad(swiglu(g_static, u_static), (g_static, u_static), dy_static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                      # a single stream, no parallel branches
            y = swiglu(g_static, u_static)
            dg, du = torch.autograd.grad(y, (g_static, u_static), dy_static)
        for seed in (3701, 3702):
            g_new, u_new, dy_new = inputs(shape, seed, dtype)
            with torch.no_grad():
                g_static.copy_(g_new), u_static.copy_(u_new), dy_static.copy_(dy_new)
            graph.replay()
            torch.cuda.synchronize()
            want = fused(g_new, u_new, dy_new)
            assert torch.equal(bits(y), bits(want[0])) and torch.equal(bits(dg), bits(want[1])) and torch.equal(bits(du), bits(want[2])), (dtype, seed)


def test_compiles_to_one_graph_with_the_eager_bits():
    from torch._dynamo.utils import counters

    def f(g, u):
        return swiglu(g * 1.0, u) * 2.0 + mlp.swiglu(g, u.detach())
    for dtype in (torch.bfloat16, torch.float32):
        torch._dynamo.reset()
        counters.clear()
        g, u, dy = inputs((2, 3, 2049), 3800, dtype)
        ge, ue = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        want = f(ge, ue)
        want.backward(dy)
        gc, uc = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        before = dict(ops.act_counts)
        out = torch.compile(f, fullgraph=True, backend="aot_eager")(gc, uc)
        out.backward(dy)
        assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + 2 and ops.act_counts["bwd_launch"] == before["bwd_launch"] + 2
        assert torch.equal(bits(out), bits(want)) and torch.equal(bits(gc.grad), bits(ge.grad)) and torch.equal(bits(uc.grad), bits(ue.grad)), dtype
        assert counters["stats"]["unique_graphs"] == 1 and not counters["graph_break"], dict(counters["stats"])


# ---- the module, convert(), install() ---------------------------------------------------------------------------------------------------------------

def tiny_step(model, ids):
    """one forward and backward under bf16 autocast -> logits, loss, {name: grad}"""
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, logits = model(ids, labels=ids)
    loss.backward()
    return logits.detach().clone(), loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def tiny_model(TL):
    from llm_qat_amd import utils_quant as UQ
    return TL.load_deterministic(TL.TinyLlama(UQ, w_bits=4, a_bits=8, kv_bits=4)).cuda()


def assert_same_step(a, b):
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))                  # the output and the loss
    assert set(a[2]) == set(b[2])
    for name in a[2]:                                         # every parameter gradient; the embedding's is the input's gradient
        assert torch.equal(bits(a[2][name]), bits(b[2][name])), name


def test_the_tiny_llama_before_and_after_convert_has_equal_bits():
    import tiny_llama as TL
    model = tiny_model(TL)
    ids = TL.deterministic_batch(2, 32).cuda()
    eager = tiny_step(model, ids)
    mlps = [m for m in model.modules() if isinstance(m, TL.MLP)]
    assert len(mlps) == TL.TINY["num_hidden_layers"] and mlp.convert(model) == 0      # the harness MLP calls F.silu inline: no act_fn to go by
    for m in mlps:
        m.act_fn = F.silu                                   # ... so it is named, as LlamaMLP names it
    params = dict(model.named_parameters())
    assert mlp.convert(model) == len(mlps) and not any(isinstance(m, TL.MLP) for m in model.modules())
    assert all(p is params[n] for n, p in model.named_parameters()) and mlp.convert(model) == 0
    before = dict(ops.act_counts)
    converted = tiny_step(model, ids)
    assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + len(mlps) and ops.act_counts["bwd_launch"] == before["bwd_launch"] + len(mlps)
    assert ops.act_counts["copy_route"] == before["copy_route"]
    assert_same_step(eager, converted)


def test_a_model_built_after_install_has_the_eager_models_bits(monkeypatch):
    import tiny_llama as TL

    class NamedMLP(TL.MLP):                                  # the harness MLP with the activation named, as the reference's LlamaMLP names it
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.act_fn = torch.nn.SiLU()
    ids = TL.deterministic_batch(2, 32).cuda()
    eager = tiny_step(tiny_model(TL), ids)
    ns = types.ModuleType("modeling_stand_in")
    ns.LlamaMLP = NamedMLP
    assert mlp.install(ns) is NamedMLP and issubclass(ns.LlamaMLP, NamedMLP)
    monkeypatch.setattr(TL, "MLP", ns.LlamaMLP)             # the harness model looks its MLP class up in its module, as the reference does
    model = tiny_model(TL)
    built = [m for m in model.modules() if isinstance(m, ns.LlamaMLP)]
    assert len(built) == TL.TINY["num_hidden_layers"]
    before = dict(ops.act_counts)
    installed = tiny_step(model, ids)
    assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + len(built) and ops.act_counts["bwd_launch"] == before["bwd_launch"] + len(built)
    assert_same_step(eager, installed)


def test_the_module_in_front_of_a_quantized_down_projection():
    from llm_qat_amd.utils_quant import QuantizeLinear
    for dtype in (torch.bfloat16, torch.float32):
        torch.manual_seed(39)
        gate, up = (QuantizeLinear(256, 688, bias=False, w_bits=4, a_bits=8).cuda().to(dtype) for _ in range(2))
        down = QuantizeLinear(688, 256, bias=False, w_bits=4, a_bits=8).cuda().to(dtype)
        m = mlp.SwiGLUMLP(gate, up, down)
        x = torch.randn(2, 16, 256, device="cuda").to(dtype)
        dy = torch.randn(2, 16, 256, device="cuda").to(dtype)
        xa = x.clone().requires_grad_(True)
        ya = down(F.silu(gate(xa)) * up(xa))
        ya.backward(dy)
        want = [p.grad.clone() for p in m.parameters()]
        m.zero_grad(set_to_none=True)
        xb = x.clone().requires_grad_(True)
        before = dict(ops.act_counts)
        yb = m(xb)
        yb.backward(dy)
        assert ops.act_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.act_counts["bwd_launch"] == before["bwd_launch"] + 1
        assert torch.equal(bits(ya), bits(yb)) and torch.equal(bits(xa.grad), bits(xb.grad)), dtype
        for p, w in zip(m.parameters(), want):
            assert torch.equal(bits(p.grad), bits(w)), dtype


# ---- the caps of the CPU tier, re-derived from the chain on this device ---------------------------------------------------------------------------

def test_the_eager_chain_and_the_fused_path_sit_within_the_caps_here():
    m = R.eager_measures("cuda")
    worst = [max(v[i] for v in m.values()) for i in range(3)]
    print({k: tuple(round(t, 4) for t in v) for k, v in m.items()})
    for got, cap in zip(worst, (R.Y_CAP, R.DG_CAP, R.DU_CAP)):
        assert cap / 8 < got <= cap / 2, (worst, cap)
    for name, (g, u, dy) in R.CASES().items():
        for dtype in DTYPES:
            gd, ud, dd = g.to(dtype).cuda(), u.to(dtype).cuda(), dy.to(dtype).cuda()
            # randn_s30 is the one case whose gate reaches -88, where a dg can be a zero: fp16 is compared up to that zero's sign
            y, dg, du = assert_chain_bits(gd, ud, dd, f"{name} {dtype}", dg_zero_sign=not (dtype is torch.float16 and float(g.min()) <= -88))
            c = R.measures(y, dg, du, gd, ud, dd)
            assert c[0] <= R.Y_CAP and c[1] <= R.DG_CAP and c[2] <= R.DU_CAP, (name, dtype, c)
