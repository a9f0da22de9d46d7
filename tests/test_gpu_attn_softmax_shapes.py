"""GPU tier of the attention softmax's launch ladder (tests/row_ladder_cases.py): every class of cells -- wave or
workgroup, 16-byte or element path, each of the three register rungs, one, two and three sweeps, both sides of every boundary -- for every
dtype pair, against float64 under the caps the eager chain set, with the row statistics held to the float64 maximum and sum; fully masked
rows and special values in the rungs no other test launches; every layout a mask can be read in where it lies; a tensor beyond 2^31
elements; hipGraph capture.  tests/test_row_ladder_cases_cpu.py shows that the cases reach every class and that a miscounted slot, a
dropped group or a dropped sweep exceeds a cap on them."""
import pytest
import torch

import attn_softmax_reference as R
import row_ladder_cases as C
from test_gpu_attn_softmax import HD, PAIRS, bits, fused

pytestmark = pytest.mark.gpu

BF, H, F = torch.bfloat16, torch.float16, torch.float32
NAME = {BF: "bf16", H: "f16", F: "f32", None: "none"}
LAYOUT_PAIRS = [(BF, F), (BF, BF), (F, F)]
WORST = {}           # what the run has measured so far: (scores, mask) -> [C_y, C_dx] of the kernels, "eager" -> the fp32 chain's


def _mods():
    from llm_qat_amd import attention, ops
    return attention, ops


def place(t, offset=0):
    """t's values on the device, in storage that starts `offset` elements behind a 16-byte boundary"""
    n = t.numel()
    out = torch.empty(n + 8, dtype=t.dtype, device="cuda")[offset:offset + n].view(t.shape)
    assert out.data_ptr() % 16 == offset * t.element_size() % 16
    return out.copy_(t)


def same(a, b):
    return all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def check(x, mask, g, what, key=None):
    """forward and backward against float64 under the caps, every element compared; exact zeros under finfo.min; the stats: the float64
    maximum exactly (a maximum is exact in any order) and the float64 sum within Y_CAP 2^-24 -> (y, dx, stats)"""
    ref = R.ref64(x, mask, g)
    y, dx, stats = fused(x, mask, g)
    cy, cdx = R.c_y(y, ref), R.c_dx(dx, ref)
    print(what, "C_y", round(cy, 3), "C_dx", round(cdx, 3))
    if key is not None:
        w = WORST.setdefault(key, [0.0, 0.0])
        w[0], w[1] = max(w[0], cy), max(w[1], cdx)
    assert cy <= R.Y_CAP and cdx <= R.DX_CAP, (what, cy, cdx)
    assert y.is_contiguous() and dx.is_contiguous() and y.dtype == x.dtype and dx.dtype == x.dtype and y.shape == x.shape == dx.shape
    if mask is not None:
        masked = (mask == torch.finfo(mask.dtype).min).expand_as(y)
        masked = masked & ~masked.all(-1, keepdim=True)              # (a fully masked row is uniform)
        assert int(torch.count_nonzero(y[masked])) == 0 and int(torch.count_nonzero(dx[masked])) == 0, what
    m64, s64 = C.row_stats64(x, mask)
    assert torch.equal(stats[:, 0].double(), m64), what
    assert ((stats[:, 1].double() - s64).abs() <= R.Y_CAP * R.UNIT * s64).all(), (what, float(((stats[:, 1].double() - s64).abs() / s64).max() / R.UNIT))
    return y, dx, stats


# ---- every cell -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", list(C.all_attn_cols()))
def test_every_cell_of_the_ladder_against_float64(cols):
    """row 0 seeded so that a slot past the row that is counted, or a last group that is not, moves y by a third; row 1 of a row wider
    than a sweep so that a maximum taken without the last sweep is wrong in the stats and overflows.  The eager fp32 chain is measured
    on the same case: the caps are 4 x its largest measure, so it stays within a quarter of them"""
    x32, keep, g32 = C.attn_inputs(cols)
    for masked in (True, False):
        xe, ge, me = x32.cuda(), g32.cuda(), C.attn_mask(keep if masked else None, F, "cuda")
        ref = R.ref64(xe, me, ge)
        ye, dxe = R.eager32(xe, me, ge)
        cy, cdx = R.c_y(ye, ref), R.c_dx(dxe, ref)
        w = WORST.setdefault("eager", [0.0, 0.0])
        w[0], w[1] = max(w[0], cy), max(w[1], cdx)
        print("eager fp32 chain", cols, "masked" if masked else "no mask", "C_y", round(cy, 3), "C_dx", round(cdx, 3))
        assert cy <= R.Y_CAP / 4 and cdx <= R.DX_CAP / 4, (cols, masked, cy, cdx)
    offsets = (0, 1) if C.all_attn_cols()[cols] else (0,)
    for ds, dm in PAIRS:
        mask = C.attn_mask(keep if dm is not None else None, dm, "cuda")
        for offset in offsets:
            cell = C.cell(cols, ds, offset == 0)
            x, g = place(x32.to(ds), offset), place(g32.to(ds), offset)
            check(x, mask, g, (cols, NAME[ds], NAME[dm], offset, tuple(cell)), key=(NAME[ds], NAME[dm]))
    print("so far:", {k: [round(v, 3) for v in w] for k, w in WORST.items()})


# ---- fully masked rows and special values in the rungs no other test launches -----------------------------------------------------------------------------
@pytest.mark.parametrize("cols,offset", [(1032, 0), (8192, 0), (1025, 0), (1032, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("ds,dm", PAIRS[:5], ids=lambda d: NAME[d])
def test_masked_rows_and_a_nan_in_the_last_group(ds, dm, cols, offset):
    S = cols
    x32, keep, g32 = C.attn_inputs(S, rows=6)
    keep[0, 0, 2] = False                                            # a fully masked row: uniform, every element a tie
    keep[0, 0, 3] = False
    keep[0, 0, 3, S - 1] = True                                      # a row whose only unmasked column is the last
    x, g, mask = place(x32.to(ds), offset), place(g32.to(ds), offset), C.attn_mask(keep, dm, "cuda")
    y, dx, stats = check(x, mask, g, (S, NAME[ds], NAME[dm], offset, "masked rows"))
    P = torch.promote_types(ds, dm)
    assert (y[0, 0, 2].float() == torch.tensor(1.0 / S).to(ds).float()).all()
    assert float(stats[2, 0]) == torch.finfo(P).min and float(stats[2, 1]) == S
    ref = R.ref64(x, mask, g)
    d = (ref["g"] - (ref["g"] * ref["p"]).sum(-1, keepdim=True)) * ref["p"] * ref["inv"]
    half = (d / 2)[0, 0, 2]
    assert (dx[0, 0, 2].double() - half).abs().max() <= 2 * (2.0 ** -8 if ds != F else 1e-6) * half.abs().max()     # d / 2, not d and not 0
    assert dx[0, 0, 2].abs().max() > 0
    assert int(torch.count_nonzero(y[0, 0, 3, :-1])) == 0 and float(y[0, 0, 3, -1]) == 1.0 and float(stats[3, 1]) == 1.0
    assert int(torch.count_nonzero(dx[0, 0, 3])) == 0
    bad = x.clone() if offset == 0 else place(x, offset)
    bad[0, 0, 4, S - 1] = float("nan")                               # in the last group: NaN by position, as the chain's
    yn, dxn, stn = fused(bad, mask, g)
    ye, dxe = R.eager32(bad, mask, g)
    assert torch.equal(torch.isnan(yn), torch.isnan(ye)) and torch.equal(torch.isnan(dxn), torch.isnan(dxe))
    assert torch.isnan(yn[0, 0, 4]).all() and torch.isnan(dxn[0, 0, 4]).all()
    rows = [0, 1, 2, 3, 5]
    assert same((yn[0, 0, rows], dxn[0, 0, rows], stn[rows]), (y[0, 0, rows], dx[0, 0, rows], stats[rows]))


# ---- mask layouts: read where it lies -----------------------------------------------------------------------------------------------------------------------
def launch_alignment(mask, B, T):
    """what attn_vec asks of a mask: the base, the batch stride and the row stride the launch passes, in bytes, all multiples of 16"""
    e = mask.element_size()
    bs = mask.stride(0) if mask.shape[0] == B and B > 1 else 0
    rs = mask.stride(2) if T > 1 else 0
    return mask.data_ptr() % 16 == 0 and bs * e % 16 == 0 and rs * e % 16 == 0


def layout_inputs(B, Hh, T, S, ds, dm, seed):
    gen = torch.Generator().manual_seed(seed)
    x = place((torch.randn(B, Hh, T, S, generator=gen) * 8).to(ds))
    g = place(torch.randn(B, Hh, T, S, generator=gen).to(ds))
    keep = torch.rand(B, 1, T, S, generator=gen) < 0.7              # distinct per (batch, token)
    keep[..., 0] = True
    return x, g, C.attn_mask(keep, dm, "cuda")


def embed(values, shape, index, dm):
    """a buffer of `shape` that holds finfo.min outside the view `index` and `values` inside it -> the view"""
    buf = torch.full(shape, torch.finfo(dm).min, dtype=dm, device="cuda")
    buf[index] = values
    view = buf[index]
    assert view.data_ptr() == buf[index].data_ptr() and torch.equal(view, values)
    return view


@pytest.mark.parametrize("S", [1032, 4104])
@pytest.mark.parametrize("ds,dm", LAYOUT_PAIRS, ids=lambda d: NAME[d])
def test_every_mask_layout_equals_the_contiguous_masks_result(ds, dm, S):
    """bit for bit where the layout keeps the 16-byte path (the mirror of attn_vec says which), under the caps against float64 where
    the mask alone sends aligned scores down the element path; no copy but for a last stride that is not 1"""
    _, ops = _mods()
    B, Hh, T = 2, 3, 4
    x, g, batched = layout_inputs(B, Hh, T, S, ds, dm, S)
    shared = batched[:1].clone()
    assert C.cell(S, ds, True).path == "vec" and x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    want = {1: fused(x, shared.expand(B, 1, T, S).contiguous(), g), B: fused(x, batched, g)}
    Tm, Sm, So = T + 3, S + 24, S + 25
    sl = slice(None)
    layouts = [
        ("cache slice, row stride a multiple of 16 bytes", embed(shared, (1, 1, Tm, Sm), (sl, sl, slice(Tm - T, None), slice(0, S)), dm), True, 0),
        ("cache slice, odd row stride", embed(shared, (1, 1, Tm, So), (sl, sl, slice(Tm - T, None), slice(0, S)), dm), False, 0),
        ("base one element off", embed(shared, (1, 1, T, S + 1), (sl, sl, sl, slice(1, S + 1)), dm), False, 0),
        ("a true [1, 1, T, S] beside B = 2", shared, True, 0),
        ("a batch stride of two masks", embed(batched, (B, 2, T, S), (sl, slice(1, 2)), dm), True, 0),
        ("a last stride of 2", embed(batched, (B, 1, T, 2 * S), (sl, sl, sl, slice(0, None, 2)), dm), True, 1),
    ]
    assert layouts[0][1].stride(2) == Sm != S and layouts[4][1].stride(0) == 2 * T * S and layouts[5][1].stride(3) == 2
    element = []
    for name, mask, vec, copies in layouts:
        assert tuple(mask.shape) in ((1, 1, T, S), (B, 1, T, S)), name
        seen = mask.contiguous() if copies else mask
        assert launch_alignment(seen, B, T) == vec, name
        before = dict(ops.attn_counts)
        y, stats = ops.attn_softmax_forward(x, mask, HD)
        assert ops.attn_counts["copy_route"] == before["copy_route"] + copies, name
        dx = ops.attn_softmax_backward(g, x, mask, stats, HD)
        assert ops.attn_counts["copy_route"] == before["copy_route"] + 2 * copies, name        # one counted copy a launch
        assert ops.attn_counts["fwd_launch"] == before["fwd_launch"] + 1 and ops.attn_counts["bwd_launch"] == before["bwd_launch"] + 1
        if vec:
            assert same((y, dx, stats), want[mask.shape[0]]), name
        else:
            got = check(x, mask, g, (S, NAME[ds], NAME[dm], name))
            assert same(got, (y, dx, stats)), name
            element.append(got)
    assert len(element) == 2 and same(*element)                      # the element path twice, by the stride and by the base: one result


@pytest.mark.parametrize("ds,dm", LAYOUT_PAIRS, ids=lambda d: NAME[d])
def test_decode_on_the_16_byte_path(ds, dm):
    """T = 1 at 1032 columns: the row stride passed is 0 whatever the mask's, and the rows are those of a launch with T = H"""
    B, Hh, S = 2, 3, 1032
    x, g, mask = layout_inputs(B, Hh, 1, S, ds, dm, 77)
    got = check(x, mask, g, (S, NAME[ds], NAME[dm], "decode"))
    rows = fused(x.view(B, 1, Hh, S), mask.expand(B, 1, Hh, S).contiguous(), g.view(B, 1, Hh, S))
    assert same(got, (rows[0].view_as(x), rows[1].view_as(x), rows[2]))
    one = mask[:1].clone()
    cache = embed(one, (1, 1, 5, S + 24), (slice(None), slice(None), slice(4, 5), slice(0, S)), dm)      # the last row of a cached mask
    assert cache.stride(2) == S + 24 and launch_alignment(cache, B, 1)
    assert same(fused(x, cache, g), fused(x, one.expand(B, 1, 1, S).contiguous(), g))


@pytest.mark.parametrize("S", [1032, 4104])
def test_a_mask_row_is_the_tokens_own_on_the_wave_full_rung_and_the_workgroup_path(S):
    """distinct masks per (batch, token): y is 0 exactly where that token's mask is negative, in every head"""
    for ds, dm in LAYOUT_PAIRS:
        x, g, mask = layout_inputs(2, 3, 4, S, ds, dm, S + 1)
        y, _, _ = fused(x, mask, g)
        assert torch.equal(y == 0, (mask < 0).expand_as(y)), (ds, dm)
        assert not torch.equal(mask[0], mask[1]) and not torch.equal(mask[0, 0, 0], mask[0, 0, 1])


# ---- beyond 2^31 elements -----------------------------------------------------------------------------------------------------------------------------------
def test_a_tensor_beyond_2_31_elements():
    """bf16 scores [1, 1025, 1024, 2056] under an fp32 [1, 1, 1024, 2056] mask: the workgroup path, more than 2^20 rows through the mask
    row's index, row * cols beyond 32 bits.  The summation order is a function of cols alone, so the first and the last eight rows must
    equal, bit for bit, the same kernels run on those rows alone; one of those small launches is held to float64"""
    Hh, T, S = 1025, 1024, 2056
    if torch.cuda.mem_get_info()[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory")
    assert C.cell(S, BF, True) == ("vec", 256, 16, 1, 257)
    x = torch.randn(1, Hh, T, S, device="cuda", dtype=BF).mul_(8)
    assert x.numel() > 2 ** 31 and Hh * T > 2 ** 20
    gen = torch.Generator().manual_seed(31)
    keep = torch.rand(1, 1, T, S, generator=gen) < 0.7
    keep[..., 0] = True
    mask = C.attn_mask(keep, F, "cuda")
    _, ops = _mods()
    y, stats = ops.attn_softmax_forward(x, mask, HD)
    ends = [(slice(0, 1), slice(0, 8), slice(0, 8)), (slice(Hh - 1, Hh), slice(T - 8, T), slice(Hh * T - 8, Hh * T))]
    kept = [(y[:, h, t].clone(), stats[r].clone()) for h, t, r in ends]
    del y
    g = torch.randn(1, Hh, T, S, device="cuda", dtype=BF)
    dx = ops.attn_softmax_backward(g, x, mask, stats, HD)
    for (h, t, r), (ys, sts) in zip(ends, kept):
        xs, gs, ms = x[:, h, t].contiguous(), g[:, h, t].contiguous(), mask[:, :, t]
        small = fused(xs, ms, gs)
        assert same((ys, dx[:, h, t], sts), small), (h, t)
    check(xs, ms, gs, "the last eight rows alone")
    del dx, g, x


# ---- hipGraph ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1032, 4104])
def test_a_captured_forward_and_backward_replays_bit_for_bit(S):
    attention, _ = _mods()
    B, Hh, T = 2, 2, 4
    x, g, mask = layout_inputs(B, Hh, T, S, BF, F, 2300 + S)
    x.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture
        torch.autograd.grad(attention.attn_softmax(x, mask, HD), x, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # a single stream, no parallel branches
        y = attention.attn_softmax(x, mask, HD)
        (dx,) = torch.autograd.grad(y, x, g)
    for seed in (2301, 2302):
        xn, gn, mn = layout_inputs(B, Hh, T, S, BF, F, seed + S)
        with torch.no_grad():
            x.copy_(xn), g.copy_(gn), mask.copy_(mn)
        graph.replay()
        torch.cuda.synchronize()
        want = fused(xn, mn, gn)
        assert torch.equal(bits(y), bits(want[0])) and torch.equal(bits(dx), bits(want[1])), (S, seed)
        assert not torch.equal(bits(y), bits(fused(xn, mask.roll(1, 2).contiguous(), gn)[0]))      # the mask's new contents were read
