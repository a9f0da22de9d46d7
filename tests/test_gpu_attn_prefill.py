"""GPU tier of the fused prefill attention (llm_qat_amd.attention.prefill_attention): the kernel against the float64
chain under tests/attn_prefill_reference.py's cap, at every query-tile and key-tile boundary."""
import copy

import pytest
import torch

from llm_qat_amd import _lib, attention, ops

import attn_prefill_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FH = torch.bfloat16, torch.float16
QT, KT = R.QT, R.KT


def fused(q, k, v, mask, D, causal=False):
    with torch.no_grad():
        return attention.prefill_attention(q, k, v, mask, D, causal=causal)


def measure(q, k, v, mask, D, causal=False, ref_mask=None):
    return R.c_out(fused(q, k, v, mask, D, causal), *R.ref64(q, k, v, mask if ref_mask is None else ref_mask, R.inv_of(D)))


@pytest.mark.parametrize("D,dtype,kind", R.DIMS)
def test_every_tile_boundary_is_within_the_cap(D, dtype, kind):
    seen = []
    for T, S in R.cases(kind):
        q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, DEV)
        seen.append((measure(q, k, v, mask, D, causal, ref_mask), T, S))
    print("fused C_out", D, dtype, kind, max(seen), "over", len(seen), "cases")
    assert all(c <= R.CAP for c, _, _ in seen), [x for x in seen if not x[0] <= R.CAP]


@pytest.mark.parametrize("D,dtype,kind", [(64, BF, "f32"), (128, FH, "ds"), (128, BF, "ds")])
def test_mask_rows_against_float64(D, dtype, kind):
    """two query tiles; batch element 1 left-padded so far that its row 0 is fully masked (the mean of v); in the second tile a -inf row
    and a row whose only unmasked key is the last"""
    T, S = QT + 5, QT + 75
    q, k, v = R.inputs(T, S, D, dtype, DEV, signed_v=True)
    mask = R.mask_of(kind, T, S, dtype, DEV, pad=S - T + 1)
    mask[0, 0, QT + 1] = float("-inf")
    mask[0, 0, QT + 2, :-1] = torch.finfo(mask.dtype).min
    mask[0, 0, QT + 2, -1] = 0
    out = fused(q, k, v, mask, D)
    assert R.c_out(out, *R.ref64(q, k, v, mask, R.inv_of(D))) <= R.CAP
    assert ((out[0, :, QT + 2].double() - v[0, :, -1].double()).abs() <= R.U[dtype] * v[0, :, -1].double().abs()).all()
    if (dtype, kind) != (FH, "ds"):      # fp16 beside an fp16 mask: finfo.min + x can round above finfo.min, so that row is not uniform
        assert ((out[1, :, 0].double() - v.double().mean(2)[1]).abs() <= R.CAP * R.U[dtype] * v.double().abs().mean(2)[1]).all()


@pytest.mark.parametrize("where", ["mask", "q"])
def test_a_nan_in_the_last_key_tile_of_the_second_query_tile_poisons_its_row_and_no_other(where):
    T, S, D, row = QT + 5, QT + 75, 128, QT + 3
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask = R.mask_of("f32", T, S, BF, DEV)
    clean = fused(q, k, v, mask, D)
    (mask[1, 0, row, -1:] if where == "mask" else q[1, 2, row, 5:6]).fill_(float("nan"))
    out = fused(q, k, v, mask, D)
    bad = torch.zeros(R.B, R.H, T, dtype=torch.bool, device=DEV)
    bad[1, slice(None) if where == "mask" else 2, row] = True
    assert torch.equal(out.isnan().all(-1), bad) and torch.equal(out.isnan().any(-1), bad) and torch.equal(out[~bad], clean[~bad])


@pytest.mark.parametrize("D,dtype", [(128, BF), (64, FH)])
def test_layouts_are_read_where_they_lie(D, dtype):
    T, P = 19, 40
    q, k, v = R.inputs(T, T, D, dtype, DEV)
    mask = R.mask_of("f32", T, T, dtype, DEV)
    views = [t.transpose(1, 2).reshape(R.B, T, R.H * D).contiguous().view(R.B, T, R.H, D).transpose(1, 2) for t in (q, k, v)]   # of a [B, T, H * D] projection
    assert not views[0].is_contiguous() and torch.equal(fused(*views, mask, D), fused(q, k, v, mask, D))
    past_k, past_v = R.inputs(T, P, D, dtype, DEV, seed=1)[1:]
    kc, vc = torch.cat([past_k, views[1]], 2), torch.cat([past_v, views[2]], 2)
    mc = R.mask_of("f32", T, P + T, dtype, DEV)
    got = fused(views[0], kc, vc, mc, D)
    assert measure(views[0], kc, vc, mc, D) <= R.CAP and torch.equal(got, fused(views[0].contiguous(), kc.contiguous(), vc.contiguous(), mc, D))
    off = [torch.empty(t.numel() + 1, dtype=dtype, device=DEV)[1:].view(t.shape).copy_(t) for t in (views[0], kc, vc, mc.to(dtype))]      # the element paths
    assert off[1].data_ptr() % 16 and torch.equal(fused(*off, D), fused(views[0], kc, vc, mc.to(dtype), D))
    before = ops.prefill_counts["copy_route"]
    strided = torch.empty(*kc.shape, 2, dtype=dtype, device=DEV)[..., 0].copy_(kc)
    assert torch.equal(fused(views[0], strided, vc, mc, D), got) and ops.prefill_counts["copy_route"] == before + 1


def test_two_calls_give_the_same_bits_and_nothing_else_is_written():
    T, S, D = QT + 1, QT + KT + 1, 128
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask = R.mask_of("ds", T, S, BF, DEV)
    flat = ops.attn_prefill_forward(q, k, v, mask, D)
    assert flat.shape == (R.B, T, R.H, D) and flat.is_contiguous() and torch.equal(flat, ops.attn_prefill_forward(q, k, v, mask, D))
    assert fused(q, k, v, mask, D).transpose(1, 2).is_contiguous()
    out = torch.full((flat.numel() + 64,), 7.0, dtype=BF, device=DEV)
    rc = ops._launch(q, _lib.lib().fqp_attn_prefill_fwd, q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr(), out.data_ptr() + 64,
                     *q.stride()[:3], *k.stride()[:3], *v.stride()[:3], mask.stride(0), mask.stride(2), R.B, R.H, T, S, D, R.inv_of(D), 1, 1, 0)
    assert rc == 0, _lib.lib().fq_last_error()
    assert torch.equal(out[32:-32].view_as(flat), flat) and (out[:32] == 7).all() and (out[-32:] == 7).all()


def test_prefill_and_decode_agree_at_sixteen_rows_over_a_cache():
    T, S, D = 16, 280, 128
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask = R.mask_of("f32", T, S, BF, DEV)
    ref = R.ref64(q, k, v, mask, R.inv_of(D))
    with torch.no_grad():
        assert R.c_out(fused(q, k, v, mask, D), *ref) <= R.CAP and R.c_out(attention.decode_attention(q, k, v, mask, D), *ref) <= R.CAP


def test_a_required_gradient_is_refused_and_the_compiled_call_equals_eager():
    q, k, v = R.inputs(QT + 1, QT + 1, 128, BF, DEV)
    with pytest.raises(RuntimeError, match="forward only"):
        attention.prefill_attention(q, k.requires_grad_(True), v, None, 128)
    k.requires_grad_(False)
    fn = torch.compile(lambda a, b, c: attention.prefill_attention(a, b, c, None, 128, causal=True) * 1, fullgraph=True)
    with torch.no_grad():
        assert torch.equal(fn(q, k, v), fused(q, k, v, None, 128, causal=True))


def test_a_two_layer_model_generates_through_both_fused_paths():
    """a prompt of 70 tokens (2 prefill launches), then 3 single-token steps with the cache (6 decode launches), no fallback in either
    dict; every step within 4 x the composed path's own relative L2 distance to the float64 CPU run"""
    from test_attn_softmax_cpu import _stub_namespace
    torch.manual_seed(5)
    base = torch.nn.ModuleList([_stub_namespace().LlamaAttention(hidden=128, heads=2) for _ in range(2)])
    for layer in base:
        layer.rotary_emb = type(layer.rotary_emb)(64, n=128)      # the stub's table ends at 64 positions
    base, hs = base.bfloat16(), [torch.randn(2, n, 128).bfloat16() for n in (70, 1, 1, 1)]

    def run(dev, dt, **convert):
        model = copy.deepcopy(base).to(dev).to(dt)
        if dev == DEV:
            attention.convert(model, **convert)
        past, outs, n = [None, None], [], 0
        for h in hs:
            h, t = h.to(dev).to(dt), h.shape[1]
            mask = torch.full((t, n + t), torch.finfo(torch.float32).min, device=dev).triu(n + 1).expand(2, 1, t, n + t).to(torch.float64 if dt == torch.float64 else torch.float32)
            for i, layer in enumerate(model):
                o, _, past[i] = layer(h, attention_mask=mask, position_ids=torch.arange(n, n + t, device=dev).expand(2, t), past_key_value=past[i], use_cache=True)
                h = h + o
            outs.append(h.double().cpu())
            n += t
        return outs

    with torch.no_grad():
        want, dec, pre = run("cpu", torch.float64), dict(ops.decode_counts), dict(ops.prefill_counts)
        got = run(DEV, BF, decode=True, prefill=True)
        assert ops.prefill_counts == dict(pre, fwd_launch=pre["fwd_launch"] + 2) and ops.decode_counts == dict(dec, fwd_launch=dec["fwd_launch"] + 6)
        for g, p, w in zip(got, run(DEV, BF), want):
            dist = [float((x - w).norm() / w.norm()) for x in (g, p)]
            print("relative L2: fused", dist[0], "composed", dist[1])
            assert dist[0] <= 4 * dist[1]


def test_peak_memory_stays_below_one_scores_tensor():
    B, H, T, D = 1, 8, 1024, 128
    q, k, v = (torch.randn(B, H, T, D, device=DEV).bfloat16() for _ in range(3))
    mask = torch.zeros(1, 1, T, T, device=DEV).masked_fill(torch.ones(T, T, dtype=torch.bool, device=DEV).triu(1), torch.finfo(torch.float32).min)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fused(q, k, v, mask, D)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base - out.numel() * 2 < B * H * T * T * 2
