"""CPU tier of the register-ladder tests (tests/row_ladder_cases.py): the cases are worth running.  The mirror's constants are the headers'
and the ladder in the sources still reads as mirrored; the case lists reach every class of cells the mirror can produce, per kernel
family and dtype, with both sides of every boundary; and SEEDED FAULTS in a float64 softmax and a float64 sum of squares -- a slot past
the row counted as a copy of the sweep's first group, the last group left out of the sum, the last sweep left out of the maximum --
exceed the caps of tests/attn_softmax_reference.py and tests/rms_norm_reference.py on every case's seeded rows, while the unmutated
float64 recipe measures nothing.  So a pass of the GPU tier means something.  No kernel runs, and the caps are not measured again here:
they were taken from the eager chain on the MI355X, and ATen's CPU kernels measure about three times higher."""
import os
import re

import pytest
import torch

import attn_softmax_reference as A
import rms_norm_reference as N
import row_ladder_cases as C

BF, H, F = C.BF, C.H, C.F
IDS = {BF: "bf16", H: "f16", F: "f32"}
dtypes = pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: IDS[d])

# the constants the lists below were worked out at: a retuned macro fails here first, and the lists are then derived again
TODAY = dict(ROW_WIDE=2048, ROW_TPB=256, ATTN_VIF=4, ATTN_EG=16, RMS_VIF=4, RMS_EG=16)
ALIGNED_16BIT = [8, 512, 520, 1024, 1032, 2040, 2048, 4096, 4104, 8192, 8200, 16392]
ELEMENT = [1, 1023, 1024, 1025, 2047, 2048, 4096, 4097, 8193]
ALIGNED_F32_ONLY = [516, 1028, 2044, 4100, 8196]


def source(name):
    return re.sub(r"\s+", " ", open(os.path.join(C.CSRC, name)).read())


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_constants_are_the_headers():
    assert C.K == C.header_constants() == TODAY
    rows = source("fq_rows.h")
    assert "inline bool row_wide(int64_t cols) { return cols >= ROW_WIDE; }" in rows
    assert "cols * esize_of(dtype) % 16 == 0" in rows and "static_assert(ROW_TPB == 256" in rows
    assert f"launch_rows<{C.WAVE} / {C.K['ROW_TPB']}>" in rows                                  # a row that is not wide takes a wave


@pytest.mark.parametrize("family,hip,head", [("attn", "fq_attn_softmax.hip", "fq_attn_softmax.h"), ("rms", "fq_rms_norm.hip", "fq_rms_norm.h")])
def test_the_ladder_in_the_sources_reads_as_mirrored(family, hip, head):
    """the lines geometry() mirrors, word for word: a ladder written another way fails here, and the mirror is then written again"""
    s, h = source(hip), source(head)
    vif, eg = (n for n in C.FAMILY[family])
    assert "need = (cols * Ty<" in s and "::ESIZE / 16 + TPR - 1) / TPR;" in s
    assert f"if (need <= {family}_groups(MOST, 2))" in s and f"else if (need <= {family}_groups(MOST, 1))" in s
    assert f"constexpr int {family}_most_groups() {{ return {vif} * Ty<DT>::ESIZE / 2; }}" in h
    assert f"constexpr int {family}_groups(int most, int step) {{ return (most >> step) > 0 ? most >> step : 1; }}" in h
    assert f"static constexpr int NG = VEC ? NGV : {eg};" in h and "static constexpr int EPV = VEC ? 16 / " in h
    assert "static constexpr int64_t SWEEP = (int64_t)NS * TPR;" in h


def test_the_mirror_at_the_counts_worked_by_hand():
    cell = C.cell
    assert cell(512, BF, True) == ("vec", 64, 8, 1, 64) and cell(520, BF, True) == ("vec", 64, 16, 1, 65)
    assert cell(1032, H, True) == ("vec", 64, 32, 1, 129) and cell(2040, BF, True) == ("vec", 64, 32, 1, 255)
    assert cell(2048, BF, True) == ("vec", 256, 8, 1, 256) and cell(2056, BF, True) == ("vec", 256, 16, 1, 257)
    assert cell(8192, BF, True) == ("vec", 256, 32, 1, 1024) and cell(8200, BF, True) == ("vec", 256, 32, 2, 1)
    assert cell(16392, F, True) == ("vec", 256, 32, 3, 2) and cell(16388, F, True) == ("vec", 256, 32, 3, 1)
    assert cell(516, F, True) == ("vec", 64, 16, 1, 129) and cell(516, BF, True) == ("elt", 64, 16, 1, 516)
    assert cell(1025, BF, False) == ("elt", 64, 16, 2, 1) and cell(4097, F, True) == ("elt", 256, 16, 2, 1)
    assert cell(8193, BF, True, "rms") == ("elt", 256, 16, 3, 1) and cell(8192, F, True, "rms") == ("vec", 256, 32, 1, 2048)


# ---- the case lists -----------------------------------------------------------------------------------------------------------------------
def reached(dtype):
    vec, elt = C.attn_cols(dtype)
    return {C.cell_class(C.cell(c, dtype, True)) for c in vec if c * C.ESIZE[dtype] % 16 == 0} | {C.cell_class(C.cell(c, dtype, False)) for c in elt}


@dtypes
def test_the_softmax_cases_reach_every_class_and_both_sides_of_every_boundary(dtype):
    all_classes = C.classes(dtype)
    assert reached(dtype) == set(all_classes) and len(all_classes) == 13
    print(IDS[dtype], sorted(all_classes.items()))
    vec, elt = C.attn_cols(dtype)
    for path, cols, step in (("vec", vec, 16 // C.ESIZE[dtype]), ("elt", elt, 1)):
        spans = sorted(v for k, v in all_classes.items() if k[0] == path)
        if path == "elt":                                            # one and several sweeps for both TPR
            assert {k[1:] for k in all_classes if k[0] == path} >= {(tpr, 16, s) for tpr in (64, 256) for s in (1, 2)}
        for (first, last), (nxt, _) in zip(spans, spans[1:] + [(None, None)]):
            assert first in cols and (nxt is None or (last in cols and nxt == last + step)), (path, first, last, nxt)
    # every rung at both TPR in one sweep; two and three sweeps of the 16-byte path with a single group in the last
    assert {k for k in all_classes if k[0] == "vec" and k[3] == 1} == {("vec", tpr, slots, 1) for tpr in (64, 256) for slots in (8, 16, 32)}
    for sweeps in (2, 3):
        first = all_classes[("vec", 256, 32, sweeps)][0]
        assert C.cell(first, dtype, True) == ("vec", 256, 32, sweeps, 1) and first in vec
    assert C.rows_of(2047) == 5 and C.rows_of(2048) == 3


def test_the_softmax_lists_hold_what_the_ladder_gives_today():
    """the counts worked by hand from the sources, and beside them the far side of two boundaries that list left open (2048 | 2056,
    16384 | 16392), the smallest fp32 row and its far sides (4, 2052, 16388) and the counts below the element path's aligned ends"""
    for dtype in (BF, H):
        vec, elt = C.attn_cols(dtype)
        assert vec == sorted(ALIGNED_16BIT + [2056, 16384]) and elt == sorted(ELEMENT + [4095, 8191, 8192])
    vec, elt = C.attn_cols(F)
    assert vec == sorted(ALIGNED_16BIT + [2056, 16384] + ALIGNED_F32_ONLY + [4, 2052, 16388]) and elt == sorted(ELEMENT + [4095, 8191, 8192])
    every = C.all_attn_cols()
    assert set(every) == set(vec) | set(elt) and {c for c, off in every.items() if off} == set(elt)


@dtypes
def test_the_norms_shapes_and_the_new_ones_reach_every_class(dtype):
    import test_gpu_rms_norm as T
    new = C.rms_new_cols(dtype)
    assert new == ([8, 512, 520, 1024, 1032, 2040, 8192, 16392] if dtype is not F else [4, 8, 512, 516, 520, 1024, 1028, 1032, 2040, 2044, 8192, 16388, 16392])
    assert set(new) <= {c for _, c in T.LADDER} and all(r == C.rows_of(c) for r, c in T.LADDER)
    all_classes = C.classes(dtype, "rms")
    before = {C.cell_class(C.cell(c, dtype, True, "rms")) for _, c in T.SHAPES}
    assert ("vec", 64, 16, 1) not in before and ("vec", 64, 32, 1) not in before          # the hole: the wave path's half and full rung
    vec = before | {C.cell_class(C.cell(c, dtype, True, "rms")) for _, c in T.LADDER}
    elt = {C.cell_class(C.cell(c, dtype, False, "rms")) for _, c in T.SHAPES if c * C.ESIZE[dtype] % 16}      # by the count, or by the offset
    elt |= {C.cell_class(C.cell(c, dtype, False, "rms")) for _, c in T.OFFSET_SHAPES + T.LADDER_OFFSET}
    assert {k for k in vec if k[0] == "vec"} | {k for k in elt if k[0] == "elt"} == set(all_classes)
    spans = dict(all_classes)
    for k in [k for k in spans if k[0] == "vec" and k[1] == 64]:
        assert set(spans[k]) <= {c for _, c in T.SHAPES + T.LADDER}, k                    # both ends of every wave rung
    assert spans[("vec", 256, 32, 1)][1] == 8192 and (3, 8192) in T.LADDER


# ---- seeded faults: the softmax -------------------------------------------------------------------------------------------------------------
def softmax_paths(cols):
    """the (aligned, first column of the last sweep, columns of a group, slots past the row) a count can run under, over the dtypes"""
    out = set()
    for dtype in C.DTYPES:
        vec, elt = C.attn_cols(dtype)
        if cols in vec and cols * C.ESIZE[dtype] % 16 == 0:
            out.add((True,) + C.last_sweep(cols, dtype, True))
        if cols in elt or cols * C.ESIZE[dtype] % 16:
            out.add((False,) + C.last_sweep(cols, dtype, False))
    return sorted(out)


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "nomask"])
def test_every_seeded_softmax_fault_exceeds_a_cap_and_the_recipe_does_not(masked):
    undetected, counts = [], dict(pad=0, drop=0, max=0)
    for cols in C.all_attn_cols():
        x, keep, g = C.attn_inputs(cols, masked=masked)
        mask = C.attn_mask(keep, F)
        row = lambda t, r: None if t is None else t[:, :, r:r + 1]      # noqa: E731
        ref0 = A.ref64(row(x, 0), row(mask, 0), row(g, 0))
        p, dx, m = C.softmax_with(ref0)
        for dt in C.DTYPES:
            assert C.c_y64(p, ref0, dt) < 1e-6 and C.c_dx64(dx, ref0, dt) < 1e-6, (cols, dt)      # nothing, to float64's own rounding
        assert torch.equal(m.reshape(-1), C.row_stats64(row(x, 0), row(mask, 0))[0])

        def caught(ref, **fault):
            p, dx, _ = C.softmax_with(ref, **fault)
            return all(C.exceeds(C.c_y64(p, ref, dt), A.Y_CAP) or C.exceeds(C.c_dx64(dx, ref, dt), A.DX_CAP) for dt in C.DTYPES)
        for aligned, c0, epv, padded in softmax_paths(cols):
            what = (cols, "vec" if aligned else "elt", c0)
            if padded:                                               # a slot past the row holds the sweep's first group
                counts["pad"] += 1
                if not caught(ref0, add_cols=(c0, min(c0 + epv, cols))):
                    undetected.append(("pad",) + what)
            counts["drop"] += 1
            if not caught(ref0, drop_cols=(cols - epv, cols)):
                undetected.append(("drop",) + what)
            if c0 > 0:                                               # a wider row: row 1 holds its maximum in the last sweep
                counts["max"] += 1
                ref1 = A.ref64(row(x, 1), row(mask, 1), row(g, 1))
                wrong = C.softmax_with(ref1, max_below=c0)[2]
                if not caught(ref1, max_below=c0) or torch.equal(wrong.reshape(-1), C.row_stats64(row(x, 1), row(mask, 1))[0]):
                    undetected.append(("max",) + what)
                p1, dx1, _ = C.softmax_with(ref1)
                assert C.c_y64(p1, ref1, F) < 1e-6 and C.c_dx64(dx1, ref1, F) < 1e-6, cols
    print(counts)
    assert not undetected, undetected
    assert counts["pad"] >= 30 and counts["drop"] >= 40 and counts["max"] >= 12, counts


def test_row_0_is_seeded_as_the_faults_need():
    for cols in C.all_attn_cols():
        x, keep, g = C.attn_inputs(cols)
        first, last, thirds = C.planted_columns(cols)
        z = x[0, 0, 0] / A.HEAD_DIM ** 0.5
        order = torch.argsort(z, descending=True)
        planted = [first] + ([last] if last != first else []) + thirds
        assert set(order[:len(planted)].tolist()) == set(planted) and int(order[0]) == 0, cols
        assert float(z[0] - z[planted].min()) < 1.0 and keep[0, 0, 0, planted].all()
        assert float(torch.exp(z[planted[-1]] - torch.logsumexp(z, 0))) > 0.15          # an O(1) share of the sum each
        assert set(g[0, 0, 0].abs().argsort(descending=True)[:len(planted)].tolist()) == set(planted)
        assert keep[..., 0].all() and 0.6 < float(keep.float().mean()) < 0.8 or cols < 64
        assert torch.equal(x, x.bfloat16().float()) and torch.equal(g, g.bfloat16().float())
        far = C.far_column(cols)
        starts = {c0 for _, c0, _, _ in softmax_paths(cols)} - {0}      # of the paths the count is run under
        assert not starts or far >= max(starts)                          # in the last sweep of each of them
        if far is not None:
            assert int(x[0, 0, 1].argmax()) == far and float(x[0, 0, 1].max()) == C.FAR and bool(keep[0, 0, 1, far])


# ---- seeded faults: the norm ----------------------------------------------------------------------------------------------------------------
def test_every_seeded_sum_of_squares_fault_exceeds_the_rstd_cap_and_the_recipe_does_not():
    import test_gpu_rms_norm as T
    undetected, n = [], 0
    for rows, cols in T.LADDER + T.LADDER_OFFSET:
        x, w, g = C.rms_inputs(cols, rows)
        first, last, thirds = C.planted_columns(cols, "rms")
        top = x[0].abs().argsort(descending=True)[:2 + len(thirds)]
        assert set(top.tolist()) == {first, last, *thirds} and float(x[0].abs().max()) == 8 * C.RMS_SIGMA
        ref = N.ref64(x[:1], w, g[:1])
        sq = x[:1].double().pow(2)
        rstd = lambda ss: torch.rsqrt(ss / cols + N.EPS)              # noqa: E731
        assert N.e_rstd(rstd(sq.sum(-1)), ref) < 1e-6
        for aligned in (True, False):
            for dtype in C.DTYPES:
                if C.cell(cols, dtype, aligned, "rms").path != ("vec" if aligned else "elt"):
                    continue
                c0, epv, padded = C.last_sweep(cols, dtype, aligned, "rms")
                faults = [("drop", sq.sum(-1) - sq[:, cols - epv:].sum(-1))]
                if padded:
                    faults.append(("pad", sq.sum(-1) + sq[:, c0:c0 + epv].sum(-1)))
                for name, ss in faults:
                    n += 1
                    if not N.e_rstd(rstd(ss), ref) > N.RSTD_CAP:
                        undetected.append((name, cols, aligned, dtype))
    assert not undetected and n >= 40, (undetected, n)
