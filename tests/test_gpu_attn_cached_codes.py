"""The decode attention over an in-place K/V cache of integer codes with device lengths against the float64 chain
over each batch row's valid cache rows and its new rows, dequantized and rotated by tests/attn_kvdecode_reference.py's operands() with
key s at position s - start, under the decode kernel's cap (a query row's arithmetic is kvd_body's; only where a key is fetched from
differs), and the append of codes and divisors bit for bit.  Every cache row the kernel must not read holds poison: the container's
largest code over a divisor of 2^-3, which no valid row has (khat = vhat = 1016 or 56 against valid magnitudes up to 8), so one read past
a length or in front of a start moves `out` far beyond the cap (or to NaN in fp16)."""
import functools

import pytest
import torch

import attn_decode_reference as R
import attn_kvdecode_reference as KR
from llm_qat_amd import _lib, attention, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HKV, SMAX, SMALL, PAD = 4, 2, 1056, 64, 64
GT = [(1, 1), (4, 4), (3, 5), (2, 16)]
DIMS = [(D, dt) for D in (64, 128) for dt in (torch.bfloat16, torch.float16)]
BITS = {"int8": 8, "int4": 4}
POISON_CODE, POISON_T2, GUARD = {"int8": 127, "int4": 0x77}, 0.125, 7
NAMES = ("k_codes", "k_t2", "v_codes", "v_t2")


@pytest.fixture(scope="module", autouse=True)
def hand_the_blocks_back():
    """the pools and the guarded buffers leave free blocks of odd sizes in the caching allocator, which hands them out unsplit where less
    than 1 MiB would remain; modules behind this one that measure peak memory get blocks of their own sizes again"""
    yield
    pool.cache_clear()
    torch.cuda.empty_cache()


def lens_of(T, smax):
    """an empty cache; new keys that straddle a tile boundary; a middle whose later chunks are empty; the last row written is the cache's last"""
    return (0, 33 - T, 500 if smax == SMAX else 40, smax - T)


@functools.lru_cache(maxsize=None)
def pool(D, dtype, container, smax):
    """KR.inputs' codes and divisors of two seeds (B = 4 batch rows, its first HKV heads, smax + 16 keys) and one pair of its tables"""
    a = [KR.inputs(1, smax + 16, D, dtype, container, DEV, seed=s) for s in (0, 1)]
    both = {n: torch.cat([x[n] for x in a]) for n in NAMES}
    return {n: (t[:, :HKV].contiguous() if t.dim() == 4 else t) for n, t in both.items()}, a[0]["rotary"]


def rows(t, b, lo, hi):
    """keys lo .. hi - 1 of batch row b of a codes tensor [B, HKV, S, W] or a divisor tensor [B, S]; b a slice keeps the batch axis"""
    return t[b, :, lo:hi] if t.dim() == 4 else t[b, lo:hi]


def padded(shape, dtype, fill):
    """-> (the flat buffer with PAD guard elements on either side, its inside as `shape`)"""
    buf = torch.full((torch.Size(shape).numel() + 2 * PAD,), GUARD, dtype=dtype, device=DEV)
    buf[PAD:-PAD] = fill
    return buf, buf[PAD:-PAD].view(shape)


def case(G, T, D, dtype, container, smax, lens, starts=(0, 0, 0, 0)):
    """-> q (multiples of 1/4, row 0 positive, every head its own), the new tensors, the four caches inside guarded buffers (poison at and
    past each length and in front of each start), the buffers, and the lengths and starts on the device"""
    src, _ = pool(D, dtype, container, smax)
    bufs, caches = {}, {}
    for n in NAMES:
        shape = (B, HKV, smax, src[n].shape[3]) if src[n].dim() == 4 else (B, smax)
        bufs[n], caches[n] = padded(shape, src[n].dtype, POISON_CODE[container] if src[n].dim() == 4 else POISON_T2)
        for b, (lo, hi) in enumerate(zip(starts, lens)):
            rows(caches[n], b, lo, hi)[...] = rows(src[n], b, lo, hi)
    new = {n: torch.stack([rows(src[n], b, hi, hi + T) for b, hi in enumerate(lens)]) for n in NAMES}
    q = torch.randint(-8, 9, (B, HKV * G, T, D), generator=torch.Generator().manual_seed(G * 100 + T)).float() / 4
    q[:, :, 0] = q[:, :, 0].abs() + 0.25
    ints = [torch.tensor(x, dtype=torch.int32, device=DEV) for x in (lens, starts)]
    return q.to(dtype).to(DEV), new, caches, bufs, ints[0], ints[1]


def call(q, new, caches, dl, D, container, rotary, ds=None):
    return attention.cached_kv_decode_attention(q, *(new[n] for n in NAMES), *(caches[n] for n in NAMES), dl, D, num_bits=BITS[container], rotary=rotary,
                                                cache_starts=ds)


def check(out, q, G, T, D, dtype, container, smax, rot, lens, starts):
    src, tables = pool(D, dtype, container, smax)
    for b, (n, lo) in enumerate(zip(lens, starts)):
        S = n + T
        pos = (torch.arange(S, device=DEV) - lo).clamp(min=0)[None]
        k, v = KR.operands(*(rows(src[x], slice(b, b + 1), 0, S) for x in NAMES), container, dtype, tables if rot else None, pos if rot else None)
        mask = R.mask_of("ds", T, S, dtype, DEV, batch=1, pad=lo)
        ref, mag = R.ref64(q[b:b + 1], k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), mask, R.inv_of(D))
        assert G == 1 or not torch.equal(ref[:, 0], ref[:, 1]), "the heads of a group must differ on the reference"
        exact = (mag == 0) & (out[b:b + 1].double() == ref)      # a column whose every weighted code is 0: the bound is 0, met exactly
        c = R.c_out(out[b:b + 1], ref, torch.where(exact, 1.0, mag))
        print(f"cached codes G={G} T={T} D={D} {dtype} {container} rot={rot} len={n} start={lo}: C_out {c:.4f}")
        assert c <= R.CAP, (b, c)


@pytest.mark.parametrize("rot", [True, False], ids=["rot", "norot"])
@pytest.mark.parametrize("container", ["int8", "int4"])
@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("G,T,smax", [(G, T, SMAX) for G, T in GT] + [(4, 4, SMALL)])
def test_appends_codes_in_place_and_attends_to_each_rows_own_length(G, T, smax, D, dtype, container, rot):
    lens = lens_of(T, smax)
    q, new, caches, bufs, dl, _ = case(G, T, D, dtype, container, smax, lens)
    rotary = pool(D, dtype, container, smax)[1] if rot else None
    nsplit = ops.attn_cached_codes_workspace(B, HKV * G, T, D, smax, ops._decode_cus(q), dtype, BITS[container], HKV)[1]
    assert nsplit > 1 if smax == SMAX else nsplit == 1
    before = {n: bufs[n].clone() for n in NAMES}
    want = {n: bufs[n].clone() for n in NAMES}
    for n in NAMES:
        inside = want[n][PAD:-PAD].view(caches[n].shape)
        for b, hi in enumerate(lens):
            rows(inside, b, hi, hi + T)[...] = new[n][b]
    out = call(q, new, caches, dl, D, container, rotary)
    assert out.shape == q.shape and out.transpose(1, 2).is_contiguous()
    check(out, q, G, T, D, dtype, container, smax, rot, lens, (0,) * B)
    for n in NAMES:
        assert torch.equal(bufs[n], want[n]), f"{n}: the append, the other rows or the guard pads"
        bufs[n].copy_(before[n])
    assert torch.equal(out, call(q, new, caches, dl, D, container, rotary)), "two calls differ"


@pytest.mark.parametrize("container", ["int8", "int4"])
@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
def test_keys_in_front_of_a_start_are_not_seen_and_positions_count_from_it(D, dtype, container):
    G, T, starts = 4, 4, (0, 0, 37, 64)
    lens = lens_of(T, SMAX)
    q, new, caches, _, dl, ds = case(G, T, D, dtype, container, SMAX, lens, starts)
    out = call(q, new, caches, dl, D, container, pool(D, dtype, container, SMAX)[1], ds)
    check(out, q, G, T, D, dtype, container, SMAX, True, lens, starts)


@pytest.mark.parametrize("G,D,dtype,container,rot", [(1, 128, torch.bfloat16, "int4", True), (4, 128, torch.bfloat16, "int8", True),
                                                     (4, 64, torch.float16, "int4", False), (1, 64, torch.float16, "int8", False)])
def test_one_chunk_has_the_bits_of_kv_decode_attention_over_the_concatenation(G, D, dtype, container, rot):
    T, smax, lens = 1, 224, (0, 31, 100, 223)
    q, new, caches, _, dl, _ = case(G, T, D, dtype, container, smax, lens)
    rotary = pool(D, dtype, container, smax)[1] if rot else None
    old = {n: caches[n].clone() for n in NAMES}
    out = call(q, new, caches, dl, D, container, rotary)
    for b, n in enumerate(lens):
        cat = [torch.cat((rows(old[x], slice(b, b + 1), 0, n), new[x][b:b + 1]), 2 if old[x].dim() == 4 else 1) for x in NAMES]
        want = attention.kv_decode_attention(q[b:b + 1], *cat, None, D, num_bits=BITS[container], rotary=rotary)
        assert torch.equal(out[b:b + 1], want), b


def test_out_and_the_workspace_stay_inside_their_bounds_and_layouts_give_the_same_bits():
    G, T, D, dtype, container = 4, 3, 128, torch.bfloat16, "int4"
    lens = lens_of(T, SMAX)
    q, new, caches, bufs, dl, _ = case(G, T, D, dtype, container, SMAX, lens)
    cos, sin = pool(D, dtype, container, SMAX)[1]
    before = {n: bufs[n].clone() for n in NAMES}
    want = call(q, new, caches, dl, D, container, (cos, sin))
    after = {n: bufs[n].clone() for n in NAMES}

    def restore():
        for n in NAMES:
            bufs[n].copy_(before[n])
    restore()
    cus, H = ops._decode_cus(q), HKV * G
    nbytes = ops.attn_cached_codes_workspace(B, H, T, D, SMAX, cus, dtype, 4, HKV)[0]
    (obuf, out), (wbuf, ws) = padded((B, T, H, D), dtype, 0.0), padded((nbytes // 4,), torch.float32, 0.0)
    L = _lib.lib()
    n, c = new, caches
    rc = ops._launch(q, L.fqw_attn_cached_codes_fwd, q.data_ptr(), *(n[x].data_ptr() for x in NAMES), *(c[x].data_ptr() for x in NAMES), dl.data_ptr(), None,
                     cos.data_ptr(), sin.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, *q.stride()[:3], *n["k_codes"].stride()[:3], *n["v_codes"].stride()[:3],
                     *c["k_codes"].stride()[:3], *c["v_codes"].stride()[:3], T, T, SMAX, SMAX, cos.shape[0], B, H, HKV, T, SMAX, D, cus, R.inv_of(D), 1, 4)
    assert rc == 0, L.fq_last_error()
    assert torch.equal(out.transpose(1, 2), want)
    assert all((b[:PAD] == GUARD).all() and (b[-PAD:] == GUARD).all() for b in (obuf.float(), wbuf, *(bufs[x].float() for x in NAMES)))
    # the new codes as the transposed views of export-layout [B, T, HKV * W] bins, and one byte off 16-byte alignment
    view = {x: n[x].transpose(1, 2).reshape(B, T, -1).contiguous().view(B, T, HKV, -1).transpose(1, 2) for x in ("k_codes", "v_codes")}
    off = {}
    for x in ("k_codes", "v_codes"):
        flat = torch.empty(n[x].numel() + 1, dtype=n[x].dtype, device=DEV)
        flat[1:] = n[x].reshape(-1)
        off[x] = flat[1:].view(n[x].shape)
    for alt in (view, off):
        restore()
        assert not alt["k_codes"].is_contiguous() or alt["k_codes"].data_ptr() % 16
        assert torch.equal(call(q, dict(n, **alt), caches, dl, D, container, (cos, sin)), want)
        assert all(torch.equal(bufs[x], after[x]) for x in NAMES)
