"""The decode attention over an in-place K/V cache with device lengths against the float64 chain over the
concatenation of each batch row's valid cache rows and its new rows, under the decode kernel's cap (the arithmetic of a query row is
unchanged; only where a key is fetched from differs), and the append bit for bit.  Every cache row the kernel must not read holds poison:
k = 2.0 (the largest possible score) and v = 1024, so one read past a length moves `out` far beyond the cap."""
import pytest
import torch

import attn_decode_reference as R
from llm_qat_amd import _lib, attention, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HKV, SMAX, SMALL, PAD = 4, 2, 1056, 64, 64
GT = [(1, 1), (4, 1), (4, 4), (3, 5), (2, 16)]
DIMS = [(D, dt) for D in (64, 128) for dt in (torch.bfloat16, torch.float16)]
POISON_K, POISON_V, GUARD = 2.0, 1024.0, 7.0


def lens_of(T, smax):
    """an empty cache; new keys that straddle a tile boundary; a middle whose later chunks are empty; the last row written is the cache's last"""
    return (0, 33 - T, 500 if smax == SMAX else 40, smax - T)


def padded(shape, dtype, fill):
    """-> (the flat buffer with PAD guard elements on either side, its inside as `shape`)"""
    n = torch.Size(shape).numel()
    buf = torch.full((n + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
    buf[PAD:-PAD] = fill
    return buf, buf[PAD:-PAD].view(shape)


def case(G, T, D, dtype, smax, lens, starts=(0, 0, 0, 0)):
    """-> q, k_new, v_new, the caches inside guarded buffers (poison at and past each length and in front of each start), the lengths and
    starts on the device, and per batch row the (k, v) concatenation the reference attends over.  Per row R.inputs(T, len + T): its seeded
    rows mark the first, middle and last key.  Row 0 of q is lowered per head as in test_gpu_attn_gqa.py, so the heads of a group differ"""
    (kbuf, kc), (vbuf, vc) = padded((B, HKV, smax, D), dtype, POISON_K), padded((B, HKV, smax, D), dtype, POISON_V)
    qs, kn, vn, full = [], [], [], []
    for b, n in enumerate(lens):
        q, k, v = R.inputs(T, n + T, D, dtype, DEV, seed=b, B=1, H=HKV * G, pool=SMAX)
        k, v = k[:, :HKV], v[:, :HKV]
        kc[b, :, starts[b]:n], vc[b, :, starts[b]:n] = k[0, :, starts[b]:n], v[0, :, starts[b]:n]
        qs.append(q), kn.append(k[:, :, n:]), vn.append(v[:, :, n:]), full.append((k, v))
    q = torch.cat(qs)
    off = 0.25 * torch.randint(0, 17, (HKV * G, D), generator=torch.Generator().manual_seed(G)).float()
    off[::G] = 0.0
    q[:, :, 0] = (2.0 - off).to(dtype).to(DEV)
    ints = [torch.tensor(x, dtype=torch.int32, device=DEV) for x in (lens, starts)]
    return q, torch.cat(kn).contiguous(), torch.cat(vn).contiguous(), (kbuf, kc), (vbuf, vc), ints[0], ints[1], full


def appended(buf, new, lens):
    """the guarded cache buffer as the call must leave it: rows [len, len + T) are the new ones, every other element keeps its bits"""
    want = buf.clone()
    inside = want[PAD:-PAD].view(B, HKV, -1, new.shape[3])
    for b, n in enumerate(lens):
        inside[b, :, n:n + new.shape[2]] = new[b]
    return want


def check(out, q, full, starts, G, T, D, dtype):
    for b, (k, v) in enumerate(full):
        mask = R.mask_of("ds", T, k.shape[2], dtype, DEV, batch=1, pad=starts[b])
        ref, mag = R.ref64(q[b:b + 1], k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), mask, R.inv_of(D))
        c = R.c_out(out[b:b + 1], ref, mag)
        print(f"cached G={G} T={T} D={D} {dtype} len={k.shape[2] - T} start={starts[b]}: C_out {c:.4f}")
        assert c <= R.CAP, (b, c)


@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("G,T,smax", [(G, T, SMAX) for G, T in GT] + [(4, 4, SMALL)])
def test_appends_in_place_and_attends_to_each_rows_own_length(G, T, smax, D, dtype):
    lens = lens_of(T, smax)
    q, kn, vn, (kbuf, kc), (vbuf, vc), dl, _, full = case(G, T, D, dtype, smax, lens)
    nsplit = ops.attn_cached_workspace(B, HKV * G, T, D, smax, ops._decode_cus(q), dtype, HKV)[1]
    assert nsplit > 1 if smax == SMAX else nsplit == 1
    before, want = (kbuf.clone(), vbuf.clone()), (appended(kbuf, kn, lens), appended(vbuf, vn, lens))
    out = attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D)
    assert out.shape == q.shape and out.transpose(1, 2).is_contiguous()
    check(out, q, full, (0,) * B, G, T, D, dtype)
    assert torch.equal(kbuf, want[0]) and torch.equal(vbuf, want[1]), "the append, the other rows or the guard pads"
    kbuf.copy_(before[0]), vbuf.copy_(before[1])
    assert torch.equal(out, attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D)), "two calls differ"


@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
def test_keys_in_front_of_a_start_are_not_seen(D, dtype):
    G, T, starts = 4, 4, (0, 0, 37, 64)
    q, kn, vn, (_, kc), (_, vc), dl, ds, full = case(G, T, D, dtype, SMAX, lens_of(T, SMAX), starts)
    check(attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D, cache_starts=ds), q, full, starts, G, T, D, dtype)


def test_out_and_the_workspace_are_written_inside_their_bounds():
    G, T, D, dtype = 4, 4, 128, torch.bfloat16
    lens = lens_of(T, SMAX)
    q, kn, vn, (kbuf, kc), (vbuf, vc), dl, _, _ = case(G, T, D, dtype, SMAX, lens)
    before = (kbuf.clone(), vbuf.clone())
    want = attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D)
    kbuf.copy_(before[0]), vbuf.copy_(before[1])
    cus = ops._decode_cus(q)
    nbytes = ops.attn_cached_workspace(B, HKV * G, T, D, SMAX, cus, dtype, HKV)[0]
    (obuf, out), (wbuf, ws) = padded((B, T, HKV * G, D), dtype, 0.0), padded((nbytes // 4,), torch.float32, 0.0)
    L = _lib.lib()
    rc = ops._launch(q, L.fqu_attn_cached_fwd, q.data_ptr(), kn.data_ptr(), vn.data_ptr(), kc.data_ptr(), vc.data_ptr(), dl.data_ptr(), None, out.data_ptr(),
                     ws.data_ptr(), nbytes, *q.stride()[:3], *kn.stride()[:3], *vn.stride()[:3], *kc.stride()[:3], *vc.stride()[:3], B, HKV * G, HKV, T, SMAX, D,
                     cus, R.inv_of(D), 1)
    assert rc == 0, L.fq_last_error()
    assert torch.equal(out.transpose(1, 2), want)
    assert all((b[:PAD] == GUARD).all() and (b[-PAD:] == GUARD).all() for b in (obuf, wbuf, kbuf, vbuf))


def misaligned(t):
    """a copy of t one element off 16-byte alignment: the element path"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def test_layouts_give_the_contiguous_calls_bits():
    """caches as slices of a larger buffer, k_new / v_new as the transposed views of a [B, T, HKV D] projection, and misaligned copies"""
    G, T, D, dtype = 4, 3, 128, torch.bfloat16
    lens = lens_of(T, SMAX)
    q, kn, vn, (kbuf, kc), (vbuf, vc), dl, _, _ = case(G, T, D, dtype, SMAX, lens)
    start = (kc.clone(), vc.clone())
    want = attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D)
    proj = [t.transpose(1, 2).reshape(B, T, HKV * D).contiguous().view(B, T, HKV, D).transpose(1, 2) for t in (kn, vn)]
    sliced = [torch.full((B, HKV, SMAX + 5, D), GUARD, dtype=dtype, device=DEV)[:, :, 3:3 + SMAX] for _ in range(2)]
    off = [misaligned(t) for t in (q, kn, vn, *start)]
    for a, (c0, c1) in ((q, *proj), sliced), (tuple(off[:3]), off[3:]):
        c0.copy_(start[0]), c1.copy_(start[1])
        assert not c0.is_contiguous() or c0.data_ptr() % 16
        assert torch.equal(attention.cached_decode_attention(*a, c0, c1, dl, D), want) and torch.equal(c0, kc) and torch.equal(c1, vc)
    assert (sliced[0]._base[:, :, :3] == GUARD).all() and (sliced[0]._base[:, :, 3 + SMAX:] == GUARD).all()


def test_torch_compile_fullgraph_gives_the_eager_bits_and_the_same_cache():
    G, T, D, dtype = 4, 4, 128, torch.bfloat16
    q, kn, vn, (kbuf, kc), (vbuf, vc), dl, _, _ = case(G, T, D, dtype, SMAX, lens_of(T, SMAX))
    before = (kbuf.clone(), vbuf.clone())
    want = attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D)
    after = (kbuf.clone(), vbuf.clone())
    kbuf.copy_(before[0]), vbuf.copy_(before[1])
    fn = torch.compile(lambda *a: attention.cached_decode_attention(*a, D) * 1, fullgraph=True)
    with torch.no_grad():
        assert torch.equal(fn(q, kn, vn, kc, vc, dl), want)
    assert torch.equal(kbuf, after[0]) and torch.equal(vbuf, after[1])
    with pytest.raises(RuntimeError, match="forward only"):
        attention.cached_decode_attention(q.clone().requires_grad_(True), kn, vn, kc, vc, dl, D)
