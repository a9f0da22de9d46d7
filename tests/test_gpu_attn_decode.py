"""GPU tier of the fused decode attention (llm_qat_amd.attention.decode_attention): the kernel against the float64
chain of tests/attn_decode_reference.py under that module's cap, at every key count where a tile, a chunk or a path changes."""
import copy

import pytest
import torch

from llm_qat_amd import _lib, attention, ops

import attn_decode_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FH = torch.bfloat16, torch.float16


def nsplit(S, B=R.B, H=R.H, T=1, D=64):      # the entry point's answer for this device
    return ops.attn_decode_workspace(B, H, T, D, S, torch.cuda.get_device_properties(0).multi_processor_count, BF)


def fused(q, k, v, mask, D):
    with torch.no_grad():
        return attention.decode_attention(q, k, v, mask, D)


def measure(q, k, v, mask, D):
    ref, mag = R.ref64(q, k, v, mask, R.inv_of(D))
    return R.c_out(fused(q, k, v, mask, D), ref, mag)


@pytest.mark.parametrize("D,dtype,kind", R.DIMS)
def test_every_key_count_is_within_the_cap(D, dtype, kind):
    seen = []
    for T in R.TS:
        for S in R.key_counts(lambda S: nsplit(S)[1]):
            mask = R.mask_of(kind, T, S, dtype, DEV, batch=R.B if S % 2 else 1, pad=S // 4)      # both batch strides of the mask
            seen.append((measure(*R.inputs(T, S, D, dtype, DEV), mask, D), T, S))
    print("fused C_out", D, dtype, kind, max(seen), "over", len(seen), "cases")
    assert all(c <= R.CAP for c, _, _ in seen), [x for x in seen if not x[0] <= R.CAP]


@pytest.mark.parametrize("D,dtype,kind", [(64, BF, "f32"), (128, FH, "ds"), (128, BF, "ds")])
def test_mask_rows_against_float64(D, dtype, kind):
    """causal with a past; batch element 1 left-padded so far that its row 0 is fully masked (the mean of v); a -inf row; a row whose only
    unmasked key is the last"""
    T, S = 3, 203
    q, k, v = R.inputs(T, S, D, dtype, DEV, signed_v=True)
    mask = R.mask_of(kind, T, S, dtype, DEV, pad=S - T + 1)
    mask[0, 0, 1] = float("-inf")
    mask[0, 0, 2, :-1] = torch.finfo(mask.dtype).min
    mask[0, 0, 2, -1] = 0
    out = fused(q, k, v, mask, D)
    assert R.c_out(out, *R.ref64(q, k, v, mask, R.inv_of(D))) <= R.CAP
    assert ((out[0, :, 2].double() - v[0, :, -1].double()).abs() <= R.U[dtype] * v[0, :, -1].double().abs()).all()
    if (dtype, kind) != (FH, "ds"):      # fp16 beside an fp16 mask: finfo.min + x can round above finfo.min, so that row is not uniform
        assert ((out[1, :, 0].double() - v.double().mean(2)[1]).abs() <= R.CAP * R.U[dtype] * v.double().abs().mean(2)[1]).all()


@pytest.mark.parametrize("where", ["mask", "q"])
def test_a_nan_in_the_last_tile_poisons_its_row_and_no_other(where):
    T, S, D = 3, 4099, 128
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask = R.mask_of("f32", T, S, BF, DEV)
    clean = fused(q, k, v, mask, D)
    (mask[1, 0, 1, -1:] if where == "mask" else q[1, 2, 1, 5:6]).fill_(float("nan"))
    out = fused(q, k, v, mask, D)
    bad = torch.zeros(R.B, R.H, T, dtype=torch.bool, device=DEV)
    bad[1, slice(None) if where == "mask" else 2, 1] = True
    assert torch.equal(out.isnan().all(-1), bad) and torch.equal(out.isnan().any(-1), bad) and torch.equal(out[~bad], clean[~bad])


@pytest.mark.parametrize("D,dtype", [(128, BF), (64, FH)])
def test_layouts_are_read_where_they_lie(D, dtype):
    T, P = 3, 40
    q, k, v = R.inputs(T, T, D, dtype, DEV)
    mask = R.mask_of("f32", T, T, dtype, DEV)
    views = [t.transpose(1, 2).reshape(R.B, T, R.H * D).contiguous().view(R.B, T, R.H, D).transpose(1, 2) for t in (q, k, v)]   # of a [B, T, H * D] projection
    assert not views[0].is_contiguous() and torch.equal(fused(*views, mask, D), fused(q, k, v, mask, D))
    past_k, past_v = R.inputs(T, P, D, dtype, DEV, seed=1)[1:]
    kc, vc = torch.cat([past_k, views[1]], 2), torch.cat([past_v, views[2]], 2)
    mc = R.mask_of("f32", T, P + T, dtype, DEV)
    got = fused(views[0], kc, vc, mc, D)
    assert measure(views[0], kc, vc, mc, D) <= R.CAP
    off = [torch.empty(t.numel() + 1, dtype=dtype, device=DEV)[1:].view(t.shape).copy_(t) for t in (views[0], kc, vc)]      # the element path
    assert off[1].data_ptr() % 16 and measure(*off, mc, D) <= R.CAP and torch.equal(fused(*off, mc, D), got)
    before = ops.decode_counts["copy_route"]
    strided = torch.empty(*kc.shape, 2, dtype=dtype, device=DEV)[..., 0].copy_(kc)
    assert torch.equal(fused(views[0], strided, vc, mc, D), got) and ops.decode_counts["copy_route"] == before + 1


def test_two_calls_give_the_same_bits_and_nothing_else_is_written():
    T, S, D = 3, 4099, 128
    q, k, v = R.inputs(T, S, D, BF, DEV)
    mask = R.mask_of("ds", T, S, BF, DEV)
    flat = ops.attn_decode_forward(q, k, v, mask, D)
    assert flat.shape == (R.B, T, R.H, D) and flat.is_contiguous() and torch.equal(flat, ops.attn_decode_forward(q, k, v, mask, D))
    assert fused(q, k, v, mask, D).transpose(1, 2).is_contiguous()
    nbytes, n = nsplit(S, T=T, D=D)
    assert n > 1 and nbytes > 0
    out = torch.full((flat.numel() + 64,), 7.0, dtype=BF, device=DEV)
    ws = torch.full((nbytes + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = ops._launch(q, _lib.lib().fqd_attn_decode_fwd, q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr(), out.data_ptr() + 64, ws.data_ptr() + 128,
                     nbytes, *q.stride()[:3], *k.stride()[:3], *v.stride()[:3], mask.stride(0), mask.stride(2), R.B, R.H, T, S, D,
                     torch.cuda.get_device_properties(0).multi_processor_count, R.inv_of(D), 1, 1)
    assert rc == 0, _lib.lib().fq_last_error()
    assert torch.equal(out[32:-32].view_as(flat), flat) and (out[:32] == 7).all() and (out[-32:] == 7).all()
    assert (ws[:128] == 0x5A).all() and (ws[-128:] == 0x5A).all()


def test_one_chunk_and_many_chunks_at_the_same_key_count():
    T, S, D = 3, 600, 64
    for b, h, many in ((1, 1, True), (8, 65, False)):
        assert (nsplit(S, b, h, T, D)[1] > 1) == many
        assert measure(*R.inputs(T, S, D, FH, DEV, B=b, H=h, pool=S), None, D) <= R.CAP


def test_a_required_gradient_is_refused_and_the_compiled_call_equals_eager():
    q, k, v = R.inputs(1, 700, 128, BF, DEV)
    with pytest.raises(RuntimeError, match="forward only"):
        attention.decode_attention(q, k.requires_grad_(True), v, None, 128)
    k.requires_grad_(False)
    fn = torch.compile(lambda a, b, c: attention.decode_attention(a, b, c, None, 128) * 1, fullgraph=True)
    with torch.no_grad():
        assert torch.equal(fn(q, k, v), fused(q, k, v, None, 128))


def test_a_two_layer_model_decodes_through_the_fused_path():
    """a prefill of 17 tokens (more than the fused path serves: the two fallbacks), then 4 single-token steps with the cache (8 fused
    launches); every step within 4 x the composed path's own relative L2 distance to the float64 CPU run"""
    from test_attn_softmax_cpu import _stub_namespace
    torch.manual_seed(5)
    base = torch.nn.ModuleList([_stub_namespace().LlamaAttention(hidden=128, heads=2) for _ in range(2)]).bfloat16()
    hs = [torch.randn(2, n, 128).bfloat16() for n in (17, 1, 1, 1, 1)]

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
        want, before = run("cpu", torch.float64), dict(ops.decode_counts)
        got = run(DEV, BF, decode=True)
        assert ops.decode_counts["fwd_launch"] - before["fwd_launch"] == 8 and ops.decode_counts["fallback"] - before["fallback"] == 2
        for g, p, w in zip(got, run(DEV, BF), want):
            dist = [float((x - w).norm() / w.norm()) for x in (g, p)]
            print("relative L2: fused", dist[0], "composed", dist[1])
            assert dist[0] <= 4 * dist[1]
