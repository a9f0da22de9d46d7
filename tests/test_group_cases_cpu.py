"""CPU tier of the group-wise kernel's launch-shape tests: the case list and the inputs of tests/group_cases.py are worth running.
Structure (every launch bracket, every served group width, full / tail / in-between rows, a planted extreme in every vector slot and
element), and SEEDED FAULTS: reductions that are wrong the way a sub-wave reduction can be wrong -- a vector slot left out, a neighbouring
group leaking in, the duplicated tail reading the wrong vector, a row of a four-row workgroup given another row's data -- applied to the
oracle's view of the data must change a compared output bit, for Sym and Asym, on every dtype, for every group width.  No kernel runs."""
import numpy as np
import pytest

import group_cases as C
from group_cases import BRACKETS, EPV, GVS

DTYPES = ["bf16", "fp16", "fp32"]
KINDS = ["sym", "asym"]


def ref(bits, g, dtype, kind):
    return C.reference(bits, g, dtype, kind, 4)


differs = C.differs


def case_data(dtype, c):
    return C.cached_inputs(dtype, c)


# ---- structure ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_case_list_meets_every_bracket_width_and_tail_kind(dtype):
    cases = C.case_list(dtype)
    epv = EPV[dtype]
    for bi, b in enumerate(BRACKETS):
        for gv in GVS:
            got = {c.kind: c.nvec for c in cases if c.bracket == bi and c.gv == gv and c.rows == 5}
            multiples = [n for n in range(b.lo + 1, b.hi + 1) if n % gv == 0]
            assert len(set(got.values())) == len(got) == min(3, len(multiples)), (bi, gv, got)   # three wherever the bracket holds three
            assert all(b.lo < n <= b.hi and n % gv == 0 for n in got.values())
            assert got["full"] == b.hi == multiples[-1]
            if len(multiples) > 1:
                assert got["tail"] == multiples[0] and got["tail"] - b.lo <= gv
            if len(multiples) > 2:
                mid = got["mid"]
                assert got["tail"] < mid < b.hi and (gv == 64 or mid % 64) and mid % b.tpr
        if b.tpr == 64:
            assert {1, 3, 4, 5} <= {c.rows for c in cases if c.bracket == bi}
    for c in cases:
        assert (c.cols, c.g) == (c.nvec * epv, c.gv * epv) and c.cols % c.g == 0 and C.bracket_of(c.nvec) == c.bracket
        assert (c.tpr, c.vpt) == (BRACKETS[c.bracket].tpr, BRACKETS[c.bracket].vpt) and c.nvec <= c.tpr * c.vpt
    gs = {c.g for c in cases}
    assert gs == ({32, 64, 128, 256, 512} if dtype != "fp32" else {16, 32, 64, 128, 256})
    assert len({c.seed for c in cases}) == len(cases)


@pytest.mark.parametrize("dtype", DTYPES)
def test_train_cases_meet_every_bracket_full_and_tail(dtype):
    cases = C.train_cases(dtype)
    for bi, b in enumerate(BRACKETS):
        for gv in (4, 64):
            for rows in (5, 3):
                kinds = {c.kind: c.nvec for c in cases if c.bracket == bi and c.gv == gv and c.rows == rows}
                assert kinds["full"] == b.hi
                assert kinds.get("tail") == (b.lo + gv if b.lo + gv < b.hi else None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_extremes_visit_every_slot_and_element(dtype):
    """in every plain group the planted element IS the largest magnitude (by a factor of two) and the planted element of the other sign IS
    the other extreme; over the case list they sit in every (vector slot, element) of a group, for every gv"""
    epv = EPV[dtype]
    seen_max = {gv: set() for gv in GVS}
    seen_min = {gv: set() for gv in GVS}
    for c in C.case_list(dtype):
        ng = c.cols // c.g
        v = C.values(case_data(dtype, c), dtype).reshape(c.rows, ng, c.g)
        kind, e = C.group_plan(c.rows, c.cols, c.g, dtype, c.seed)
        pmax, pmin = C.planted_positions(c.rows, ng, c.g, dtype, c.seed)
        plain = kind == "normal"
        a = np.abs(v)
        top = np.take_along_axis(a, pmax[:, :, None], 2)[:, :, 0]
        assert (a.argmax(2) == pmax)[plain].all() and (top == 1.5 * np.exp2(e))[plain].all()
        second = np.sort(a, 2)[:, :, -2]
        assert (top >= 2 * second)[plain].all()
        sg = np.sign(np.take_along_axis(v, pmax[:, :, None], 2)[:, :, 0])
        other = np.where(sg > 0, v.argmin(2), v.argmax(2))
        assert (other == pmin)[plain].all() and (pmax // epv != pmin // epv).all()
        # neighbouring plain groups are at least 2^3 apart
        both = plain[:, 1:] & plain[:, :-1]
        with np.errstate(all="ignore"):
            ratio = top[:, 1:] / top[:, :-1]
        assert ((ratio >= 8) | (ratio <= 1 / 8))[both].all()
        if ng >= 16:
            assert np.nanmax(np.where(plain, top, np.nan)) / np.nanmin(np.where(plain, top, np.nan)) >= 2.0 ** 18   # many binades in a row
        for pm, seen in ((pmax, seen_max), (pmin, seen_min)):
            seen[c.gv] |= {(int(p) // epv, int(p) % epv) for p in pm[plain]}
    full = lambda gv: {(s, k) for s in range(gv) for k in range(epv)}  # noqa: E731
    for gv in GVS:
        assert seen_max[gv] == full(gv) and seen_min[gv] == full(gv), gv


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_groups_sit_where_the_issue_puts_them(dtype):
    """over the case list every special kind appears as a first group, as a last group (next to the duplicated tail) and next to a 16- or
    32-lane boundary; every case's special groups hold what their name says"""
    first, last, lane = set(), set(), set()
    for c in C.case_list(dtype):
        ng = c.cols // c.g
        bits = case_data(dtype, c).reshape(c.rows, ng, c.g)
        v = C.values(bits, dtype)
        kind, _ = C.group_plan(c.rows, c.cols, c.g, dtype, c.seed)
        assert set(C.special_locations(c.nvec, c.gv)) >= {0, ng - 1}
        for r, j in zip(*np.nonzero(kind != "normal")):
            k, x = kind[r, j], v[r, j]
            if j == 0:
                first.add(k)
            if j == ng - 1:
                last.add(k)
            if any(0 < b < c.nvec and b % 16 == 0 for b in (j * c.gv, (j + 1) * c.gv)):
                lane.add(k)
            if k == "nan":
                assert np.isnan(x).sum() == 1
            elif k in ("pinf", "ninf"):
                assert np.isinf(x).sum() == 1 and (x[np.isinf(x)] > 0) == (k == "pinf") and not np.isnan(x).any()
            elif k == "zero":
                assert (x == 0).all() and np.signbit(x).sum() == 1
            elif k == "maxfin":
                assert np.isfinite(x).all() and x.max() == -x.min() == C.values(np.array([C.MAXFIN[dtype]], C.uint_of(dtype)), dtype)[0]
            elif k == "subnormal":
                tiny = {"bf16": 2.0 ** -126, "fp16": 2.0 ** -14, "fp32": 2.0 ** -126}[dtype]
                assert (x != 0).all() and (np.abs(x) < tiny).all() and (x > 0).any() and (x < 0).any()
            elif k == "allpos":
                assert (x > 0).all() and len(np.unique(x)) > 2
            elif k == "allneg":
                assert (x < 0).all() and len(np.unique(x)) > 2
            elif k == "const":
                assert len(np.unique(bits[r, j])) == 1 and np.isfinite(x).all() and x[0] != 0
        # the boundary groups: wherever lane 16 / 32 / 48 / 64 of the first wave falls between two groups, both neighbours are listed
        loc = set(C.special_locations(c.nvec, c.gv))
        for b in (16, 32, 48, 64):
            if b < c.nvec and b % c.gv == 0:
                assert {b // c.gv - 1, b // c.gv} <= loc
    assert first == last == lane == set(C.KINDS), (first, last, lane)


# ---- seeded faults -----------------------------------------------------------------------------------------------------------------------

def drop_slot(bits, c, dtype, pos):
    """every group loses the vector slot that holds element pos[r, j]: the slot is overwritten with its right neighbour's contents, so the
    group's extremes become those of the other gv - 1 slots -> (faulty input, bool mask of the overwritten elements)"""
    epv = EPV[dtype]
    ng = c.cols // c.g
    x = bits.reshape(c.rows, ng, c.gv, epv).copy()
    r, j = np.meshgrid(np.arange(c.rows), np.arange(ng), indexing="ij")
    s = pos // epv
    x[r, j, s] = x[r, j, (s + 1) % c.gv]
    hit = np.zeros(x.shape, bool)
    hit[r, j, s] = True
    return x.reshape(c.rows, c.cols), hit.reshape(c.rows, c.cols)


def with_neighbour(bits, c, dtype, kind, side):
    """every group quantized with the extremes of itself AND its right (side = 1) or left (side = -1) neighbour: the oracle on rows of
    two groups; a row's outermost group has no such neighbour and keeps its own result"""
    ng = c.cols // c.g
    x = bits.reshape(c.rows, ng, c.g)
    nb = np.roll(x, -side, 1)
    if side == 1:
        nb[:, -1] = x[:, -1]
    else:
        nb[:, 0] = x[:, 0]
    pair = np.concatenate([x, nb], 2)
    return ref(pair.reshape(-1, 2 * c.g), 2 * c.g, dtype, kind).reshape(c.rows, ng, 2 * c.g)[:, :, :c.g].reshape(c.rows, c.cols)


def tail_with_first_vector(bits, c, dtype, kind):
    """the last group of every row quantized with the row's FIRST vector mixed into its extremes (what a duplicated tail slot that read
    vector 0 instead of the last one would do) -> the last groups' outputs [rows, g]"""
    epv = EPV[dtype]
    x = np.concatenate([bits[:, c.cols - c.g:], bits[:, :epv]], 1)
    return ref(x, c.g + epv, dtype, kind)[:, :c.g]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_seeded_reduction_fault_changes_a_compared_bit(dtype, kind):
    undetected = []
    slots_hit = {gv: set() for gv in GVS}
    for c in C.case_list(dtype):
        ng = c.cols // c.g
        bits = case_data(dtype, c)
        good = ref(bits, c.g, dtype, kind)
        plan, e = C.group_plan(c.rows, c.cols, c.g, dtype, c.seed)
        plain = plan == "normal"
        pmax, pmin = C.planted_positions(c.rows, ng, c.g, dtype, c.seed)

        # (1) a group extreme taken without one vector slot: EVERY plain group notices the loss of the slot of its planted maximum (and,
        # Asym, of its planted other extreme) in the elements the fault did not touch
        for pos in ((pmax,) if kind == "sym" else (pmax, pmin)):
            bad_in, hit = drop_slot(bits, c, dtype, pos)
            d = (differs(ref(bad_in, c.g, dtype, kind), good, dtype) & ~hit).reshape(c.rows, ng, c.g).any(2)
            if not d[plain].all():
                undetected.append(("slot", c, int((~d[plain]).sum())))
            slots_hit[c.gv] |= {int(s) for s in (pos // EPV[dtype])[plain & d]}

        # (2) / (3) a neighbour leaking in: every plain group next to a plain group of a larger magnitude changes
        for side in (1, -1):
            if ng < 2:
                continue
            d = differs(with_neighbour(bits, c, dtype, kind, side), good, dtype).reshape(c.rows, ng, c.g).any(2)
            nb_e, nb_plain = np.roll(e, -side, 1), np.roll(plain, -side, 1)
            must = plain & nb_plain & (nb_e > e)
            must[:, -1 if side == 1 else 0] = False
            if not d[must].all() or (c.rows == 5 and ng >= 4 and not must.any()):
                undetected.append(("neighbour", side, c))

        # (4) the tail group's extremes with the row's first vector mixed in
        if ng >= 2 and (plain[:, 0] & plain[:, -1]).any():      # (rows >= 3: group_plan keeps one such row)
            d = differs(tail_with_first_vector(bits, c, dtype, kind), good[:, c.cols - c.g:], dtype)
            if not d.any():
                undetected.append(("tail", c))

        # (5) a row at or beyond a multiple of four given the previous row's data
        for r in range(4, c.rows):
            bad_in = bits.copy()
            bad_in[r] = bits[r - 1]
            if not differs(ref(bad_in, c.g, dtype, kind), good, dtype)[r].any():
                undetected.append(("row", r, c))
    assert not undetected, undetected[:10]
    for gv in GVS:
        assert slots_hit[gv] == set(range(gv)), (gv, sorted(set(range(gv)) - slots_hit[gv]))   # for every p < gv


# ---- training mode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_training_inputs_hold_clippable_and_safe_rows_and_both_predicate_values(dtype):
    u = C.uint_of(dtype)
    two, sign = u(C.TWO[dtype]), u(C.SIGN[dtype])
    edge = [two, two | sign, two + u(1), two - u(1), (two + u(1)) | sign, (two - u(1)) | sign]
    for c in C.train_cases(dtype):
        bits = C.group_inputs(c.rows, c.cols, c.g, dtype, c.seed, train=True)
        v = C.values(bits, dtype)
        pred = C.clip_predicate(bits, dtype)
        for asym in (False, True):
            b = C.row_bounds(bits, dtype, asym)
            clippable = ~((b[:, 0] < 2.0) & (b[:, 1] > -2.0))
            assert clippable.any() and (~clippable).any(), c
            assert clippable.tolist() == [r % 2 == 0 for r in range(c.rows)]
            assert not pred[~clippable].any()
            for r in np.flatnonzero(clippable):
                assert pred[r].any() and (~pred[r]).any(), (c, r)
        has_nan = np.isnan(v).any(1)
        assert has_nan[2] and pred[2].any() and not has_nan[0]        # a clipping row with a NaN, and one without (the integer compare)
        for r in range(0, c.rows, 2):
            for pat in edge:                                         # +-2 and one ulp on either side, in every clipping row
                assert (bits[r] == pat).any(), (c, r, hex(int(pat)))
        assert [bool(x) for x in pred[0][np.isin(bits[0], edge[:2])]] == [True] * int(np.isin(bits[0], edge[:2]).sum())
        assert pred[0][bits[0] == edge[2]].all() and not pred[0][bits[0] == edge[3]].any()
        assert pred[0][bits[0] == edge[4]].all() and not pred[0][bits[0] == edge[5]].any()
