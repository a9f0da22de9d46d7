"""GPU tier of the fused training attention (llm_qat_amd.attention.train_attention): the forward and the two
backward kernels against the float64 reference under tests/attn_train_reference.py's caps, at every tile boundary of the three kernels."""
import copy

import pytest
import torch

from llm_qat_amd import _lib, attention, ops

import attn_train_reference as R
from attn_softmax_reference import UNIT, Y_CAP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FH = torch.bfloat16, torch.float16
QT, KT = max(R.QTS), max(R.KTS)


@pytest.mark.parametrize("D,dtype,kind", R.DIMS)
def test_every_tile_boundary_is_within_the_caps_and_the_stats_are_the_float64_ones(D, dtype, kind):
    """out, dq, dk, dv within the caps; the composed path on the same cases within a quarter of each; stats: the float64 maximum exactly
    and the float64 sum within section 29's bound"""
    worst = {"fused": dict.fromkeys(R.NAMES, 0.0), "composed": dict.fromkeys(R.NAMES, 0.0)}
    for T, S in R.cases(kind):
        q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, DEV)
        dout = R.dout_of(T, D, dtype, DEV)
        ref = R.ref64(q, k, v, ref_mask, R.inv_of(D), dout)
        for path, got in (("fused", R.fused(q, k, v, mask, D, dout, causal)), ("composed", R.composed(q, k, v, ref_mask, D, dout))):
            for n, c in R.measures(got, ref).items():
                worst[path][n] = max(worst[path][n], c if c == c else float("inf"))
        stats = ops.attn_train_forward(q, k, v, mask, D, causal=causal)[1]
        assert torch.equal(stats[..., 0].double(), ref["m"]), (T, S)
        assert ((stats[..., 1].double() - ref["l"]).abs() <= Y_CAP * UNIT * ref["l"]).all(), (T, S)
    print("measures", D, dtype, kind, worst)
    assert all(worst["fused"][n] <= R.CAPS[n] and worst["composed"][n] <= R.CAPS[n] / 4 for n in R.NAMES), worst


@pytest.mark.parametrize("D,dtype", [(128, BF), (64, FH)])
def test_layouts_are_read_where_they_lie(D, dtype):
    T, S = 19, 45
    q, k, v = R.inputs(T, S, D, dtype, DEV)
    mask, dout = R.mask_of("f32", T, S, dtype, DEV), R.dout_of(T, D, dtype, DEV)
    want = R.fused(q, k, v, mask, D, dout)
    views = [t.transpose(1, 2).reshape(R.B, -1, R.H * D).contiguous().view(R.B, -1, R.H, D).transpose(1, 2) for t in (q, k, v)]      # of a projection
    fusedp = torch.cat([t.transpose(1, 2).reshape(R.B, T, -1) for t in (q, k[:, :, :T], v[:, :, :T])], -1)                       # [B, T, 3 H D]
    qp, kp, vp = (t.view(R.B, T, R.H, D).transpose(1, 2) for t in fusedp.split(R.H * D, -1))
    same = lambda a, b: all(torch.equal(a[n], b[n]) for n in R.NAMES)  # noqa: E731
    before = ops.train_counts["copy_route"]
    assert not views[0].is_contiguous() and same(R.fused(*views, mask, D, dout), want)
    assert same(R.fused(q, k, v, mask, D, dout.transpose(1, 2).contiguous().transpose(1, 2)), want) and ops.train_counts["copy_route"] == before
    mt = mask[..., :T].contiguous()
    assert same(R.fused(qp, kp, vp, mt, D, dout), R.fused(q, k[:, :, :T], v[:, :, :T], mt, D, dout))
    off = [torch.empty(t.numel() + 1, dtype=dtype, device=DEV)[1:].view(t.shape).copy_(t) for t in (q, k, v, mask.to(dtype), dout)]   # the element paths
    got = R.fused(*off[:4], D, off[4])
    assert off[1].data_ptr() % 16 and same(got, R.fused(q, k, v, mask.to(dtype), D, dout))
    c = R.measures(got, R.ref64(q, k, v, mask.to(dtype), R.inv_of(D), dout))
    assert all(c[n] <= R.CAPS[n] for n in R.NAMES), c
    strided = torch.empty(*dout.shape, 2, dtype=dtype, device=DEV)[..., 0].copy_(dout)
    assert same(R.fused(q, k, v, mask, D, strided), want) and ops.train_counts["copy_route"] == before + 1


def test_two_backward_calls_give_the_same_bits_and_nothing_else_is_written():
    T, S, D, pad = QT + 1, QT + KT + 1, 128, 64
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask, dout = R.mask_of("ds", T, S, BF, DEV), R.dout_of(T, D, BF, DEV)
    flat, stats, _ = ops.attn_train_forward(q, k, v, mask, D)
    out = flat.transpose(1, 2)
    want = ops.attn_train_backward(dout, q, k, v, mask, out, stats, D)
    assert all(torch.equal(a, b) for a, b in zip(want, ops.attn_train_backward(dout, q, k, v, mask, out, stats, D)))
    assert [tuple(t.shape) for t in want] == [(R.B, T, R.H, D), (R.B, S, R.H, D), (R.B, S, R.H, D)] and all(t.is_contiguous() for t in want)
    bufs = [torch.full((n + 2 * pad,), 7.0, dtype=dt, device=DEV) for n, dt in
            ((R.B * R.H * T, torch.float32), (want[0].numel(), BF), (want[1].numel(), BF), (want[2].numel(), BF), (flat.numel(), BF), (stats.numel(), torch.float32))]
    ptr = [t.data_ptr() + pad * t.element_size() for t in bufs]
    L, args = _lib.lib(), (*q.stride()[:3], *k.stride()[:3], *v.stride()[:3])
    tail = (mask.stride(0), mask.stride(2), R.B, R.H, T, S, D, R.inv_of(D), 1, 1, 0)
    assert ops._launch(q, L.fqg_attn_train_fwd, q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr(), ptr[4], ptr[5], *args, *tail) == 0, L.fq_last_error()
    assert ops._launch(q, L.fqg_attn_train_bwd, q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr(), out.data_ptr(), dout.data_ptr(), stats.data_ptr(),
                       *ptr[:4], *args, *out.stride()[:3], *dout.stride()[:3], *tail) == 0, L.fq_last_error()
    for buf, ref in zip(bufs[1:], (*want, flat, stats)):
        assert torch.equal(buf[pad:-pad].view_as(ref), ref)
    assert all((b[:pad] == 7).all() and (b[-pad:] == 7).all() for b in bufs) and torch.isfinite(bufs[0][pad:-pad]).all()


def test_gradient_plumbing_no_grad_compile_and_the_saved_tensors():
    T, S, D = 40, 70, 64
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask, dout = R.mask_of("f32", T, S, BF, DEV), R.dout_of(T, D, BF, DEV)
    want = R.fused(q, k, v, mask, D, dout)
    for frozen in (0, 1):
        leaves = [t.clone().requires_grad_(i != frozen) for i, t in enumerate((q, k, v))]
        attention.train_attention(*leaves, mask, D).backward(dout)
        assert [t.grad is None for t in leaves] == [i == frozen for i in range(3)]
        assert all(torch.equal(t.grad, want[n]) for i, (t, n) in enumerate(zip(leaves, R.NAMES[1:])) if i != frozen)
    before = dict(ops.train_counts)
    with torch.no_grad():
        out = attention.train_attention(leaves[0], leaves[1], leaves[2], mask, D)
    assert out.grad_fn is None and torch.equal(out, want["out"]) and ops.train_counts == dict(before, fwd_launch=before["fwd_launch"] + 1)
    assert attention.train_attention(q, k, v, mask, D).grad_fn is None
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    out = attention.train_attention(*leaves, mask, D)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 6 and [tuple(t.shape) for t in saved] == [tuple(q.shape), tuple(k.shape), tuple(v.shape), (R.B, T, R.H, D), (R.B, R.H, T, 2), tuple(mask.shape)]
    fn = torch.compile(lambda a, b, c: attention.train_attention(a, b, c, mask, D) * 1, fullgraph=True)
    got = fn(*leaves)
    got.backward(dout)
    assert torch.equal(got, want["out"]) and all(torch.equal(t.grad, want[n]) for t, n in zip(leaves, R.NAMES[1:]))


def test_peak_memory_stays_below_one_scores_tensor():
    B, H, T, D = 1, 4, 1024, 64
    q, k, v = (torch.randn(B, H, T, D, device=DEV).bfloat16().requires_grad_(True) for _ in range(3))
    dout = torch.randn(B, H, T, D, device=DEV).bfloat16()
    mask = torch.zeros(1, 1, T, T, device=DEV).masked_fill(torch.ones(T, T, dtype=torch.bool, device=DEV).triu(1), torch.finfo(torch.float32).min)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    attention.train_attention(q, k, v, mask, D).backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak over the inputs and the mask:", peak, "bytes")
    assert peak < B * H * T * T * 2


def test_a_two_layer_model_takes_a_training_step_through_the_fused_route():
    """every parameter gradient's relative L2 distance from the composed route is at most twice the composed route's own distance from
    the same step in fp32 on the device: both are 16-bit paths that round at different points"""
    from test_attn_softmax_cpu import _stub_namespace
    torch.manual_seed(5)
    base = torch.nn.ModuleList([_stub_namespace().LlamaAttention(hidden=128, heads=2) for _ in range(2)])
    for layer in base:
        layer.rotary_emb = type(layer.rotary_emb)(64, n=128)      # the stub's table ends at 64 positions
    h0, t = torch.randn(2, 70, 128), 70

    def run(dt, **convert):
        model = copy.deepcopy(base).to(DEV).to(dt)
        attention.convert(model, **convert)
        h = h0.to(DEV).to(dt)
        mask = torch.full((t, t), torch.finfo(torch.float32).min, device=DEV).triu(1).expand(2, 1, t, t)
        for layer in model:
            h = h + layer(h, attention_mask=mask, position_ids=torch.arange(t, device=DEV).expand(2, t))[0]
        h.float().square().mean().backward()
        return [p.grad.double() for p in model.parameters()]

    before = dict(ops.train_counts)
    got = run(BF, train=True)
    assert ops.train_counts == dict(before, fwd_launch=before["fwd_launch"] + 2, bwd_launch=before["bwd_launch"] + 2)
    for g, c, w in zip(got, run(BF), run(torch.float32)):
        fused_d, own = float((g - c).norm() / c.norm()), float((c - w).norm() / w.norm())
        print("relative L2: fused to composed", fused_d, "composed to fp32", own)
        assert fused_d <= 2 * own
