"""CPU tier of the pitched row-kernel walk (tests/test_gpu_row_views.py): the case lists of tests/row_view_cases.py reach every launch
shape with every pairing of layouts, no case addresses outside its buffer or lets two destination rows overlap, and the layouts SEE
addressing faults -- a numpy restatement of a launch (gather the source rows through its view, store them through the destination's view
into a buffer of canaries) is run with one deliberate fault at a time, and its result must differ from the expected buffer in a compared
element or a canary.  No kernel runs.

The restated launch is the identity on rows: the rows of every input differ from one another (tests below), so a row read from or stored
to the wrong place shows as it does behind any of the kernels, whose results are functions of the row.  A faulty address outside the
allocation reads memory the test does not own: the model gives it the hostile fill, as an unknown value would almost surely differ too;
a faulty store outside the allocation shows by the canaries its due place keeps."""
import numpy as np
import pytest

import group_cases as G
import row_view_cases as V
from test_shape_tables_cpu import tables  # noqa: F401  (the fixture: the tables as the compiled header gives them)

REG_RUNGS = 14
WIDE_COUNTS = {(64, h) for h in range(1, 9)} | {(256, h) for h in range(3, 9)} | {(1024, h) for h in range(3, 9)}


def views_of(c):
    """-> [(source View, destination View, rows, source epv, destination epv)]: one entry per source of the case (fq_ste_bwd_v has two)"""
    cols = V.case_cols(c)
    se, de = V.case_epvs(c)
    rows = V.pairing_rows(c.pairing)
    names = c.pairing[1:]
    return [(V.layout(s, cols, se, rows), V.layout(names[-1], cols, de, rows), rows, se, de) for s in names[:-1]]


# ---- structure ---------------------------------------------------------------------------------------------------------------------------

def test_every_launch_shape_is_reached_by_every_pairing(tables):  # noqa: F811
    served = {n for n, ok in tables["count"].items() if ok}
    assert served == set(range(1, 9)) and len(set(tables["reg"].values())) == REG_RUNGS
    for form in V.FORMS:
        by = {}
        for c in V.cases(form):
            by.setdefault((c.dt, c.pairing[0]), []).append(c)
        names = {p for _, p in by}
        want = {p[0] for p in (V.TRIPLES if form == "bwd_rows" else V.PAIRINGS)}
        assert want <= names, (form, want - names)
        for (dt, pname), cs in by.items():
            if form in ("fwd", "fwd_ac1"):
                got = {tables["reg"][V.case_cols(c) // G.EPV[dt]] for c in cs}
                assert got == set(tables["reg"].values()), (form, dt, pname, set(tables["reg"].values()) - got)
                # ... and every rung at a width whose last lane slot is the clamped duplicate: one vector short of the rung's top
                assert all(tables["reg"][c.width] == tables["reg"][c.shape] and c.shape == c.width - 1 for c in cs)
                tops = {max(n for n, s in tables["reg"].items() if s == shape) for shape in set(tables["reg"].values())}
                assert tops <= {c.width for c in cs}
            elif form == "fwd_wide":
                got = {c.shape for c in cs}
                assert got == WIDE_COUNTS and len(got) == 20, (dt, pname, WIDE_COUNTS ^ got)
                assert all(h in served and c.width == tpr * h - 2 for c in cs for tpr, h in [c.shape])
            else:
                assert {c.shape for c in cs} == served, (form, dt, pname, {c.shape for c in cs})
    assert len(V.WIDE_NH) == 20 and sorted(V.backward_vpt(n - 1) for n in V.MASK_BWD_NVECS) == list(range(1, 9))
    assert {V.rows_vpt(n) for n in V.ROW_NVECS} == served and V.rows_vpt(2049) == 5


def test_the_pairings_hold_every_combination_the_walk_promises():
    p = {name: (s, d) for name, s, d in V.PAIRINGS}
    assert any(s != "contig" and d == "contig" for s, d in p.values())                                  # pitched source, contiguous destination
    assert any(s == "contig" and d != "contig" for s, d in p.values())                                  # contiguous source, pitched destination
    assert any("contig" not in (s, d) and s != d and s in V.LAYOUTS_2D for s, d in p.values())          # both pitched, different views
    assert ("transposed", "padded") in p.values() and ("padded", "transposed") in p.values()            # both 3-D orders, as source and as destination
    assert any(s == "expanded" for s, d in p.values()) and all(d != "expanded" for s, d in p.values())  # expanded rows: sources only
    assert all(t[3] != "expanded" for t in V.TRIPLES)
    for cols, epv in ((56, 8), (28, 4)):
        t, q = V.layout("transposed", cols, epv), V.layout("padded", cols, epv)
        assert t.n_inner == q.n_inner == 3 and t.stride_outer < t.stride_inner and q.stride_outer > q.stride_inner > cols
        h = V.layout("half", 56, 8)
        assert h.offset % 8 == 4 and h.stride_inner % 8 == 4


# the tensors the layouts are views of, in elements: what an allocation of the described tensor holds
TENSOR_ELEMS = {"contig": lambda r, c, e: r * c, "slice": lambda r, c, e: r * (c + 3 * e), "every_other": lambda r, c, e: 2 * r * c,
                "expanded": lambda r, c, e: c + 3 * e, "half": lambda r, c, e: r * (c + 12), "transposed": lambda r, c, e: 6 * (c + 2 * e),
                "padded": lambda r, c, e: 2 * (3 * (c + 2 * e) + e) + 2 * e}


@pytest.mark.parametrize("form", V.FORMS)
def test_addresses_stay_inside_the_buffers_and_destination_rows_apart(form):
    for c in V.cases(form):
        cols = V.case_cols(c)
        names = c.pairing[1:]
        for i, (sv, dv, rows, se, de) in enumerate(views_of(c)):
            for v, epv, name, is_dst in ((sv, se, names[i], False), (dv, de, names[-1], True)):
                st = V.row_starts(v, rows, cols)
                assert st.min() >= 0 and V.buffer_elems(v, rows, cols) == st.max() + cols <= TENSOR_ELEMS[name](rows, cols, epv), (c, name)
                if name == "half":
                    assert (st % 4 == 0).all() and (st % 8 == 4).any(), (c, st)
                else:
                    assert (st % epv == 0).all(), (c, name, st)
                if is_dst:
                    s = np.sort(st)
                    assert (np.diff(s) >= cols).all(), (c, name, "destination rows overlap")


def test_rows_of_every_input_differ_from_one_another():
    for dt in ("bf16", "fp16", "fp32"):
        for cols in (63 * G.EPV[dt], 8191 * G.EPV[dt]):
            for rows in (5, 6):
                b = V.row_bits(dt, cols, rows)
                g = V.grad_and_masked(dt, cols, rows)[0]
                for a in (b, g):
                    # ... in their first and in their last vector too (what a store one vector past the row's end would leave behind)
                    for part in (a, a[:, : G.EPV[dt]], a[:, -G.EPV[dt]:]):
                        assert len({r.tobytes() for r in part}) == rows, (dt, cols, rows)
                assert all((b[r, -G.EPV[dt]:] != b[r + 1, : G.EPV[dt]]).any() for r in range(rows - 1))


def test_source_buffers_are_hostile_where_no_row_reads():
    for dt in ("bf16", "fp32"):
        epv = G.EPV[dt]
        cols = 63 * epv
        for name in ("slice", "every_other", "transposed", "padded", "expanded"):
            rows = V.rows_of(name)
            v = V.layout(name, cols, epv)
            data = V.row_bits(dt, cols, rows)
            buf, seen = V.source_buffer(data, v, dt)
            assert np.array_equal(seen, V.as_addressed(data, v))
            used = V.addressed(v, rows, cols, buf.size)
            big, nan = V.hostile(dt)
            vals = G.values(buf, dt)
            assert np.nanmax(np.abs(G.values(data, dt))) < G.values(np.array([big]), dt)[0] == 12288.0
            assert (np.isnan(vals[~used]) | (vals[~used] == 12288.0)).all()
            gaps = ~used & np.concatenate([[True], used[:-1]])
            assert gaps.sum() >= 1 and np.isnan(vals[gaps]).all() and not used[-V.GUARD:].any()


# ---- seeded addressing faults -----------------------------------------------------------------------------------------------------------

FAULTS = ("swap_strides", "swap_divmod", "n_inner_plus", "n_inner_minus", "drop_offset", "other_view", "assume_contig", "store_past_cols",
          "row4_as_3")


def faulty_starts(view, other, rows, cols, fault):
    """row_starts() with one fault seeded"""
    r = np.arange(rows, dtype=np.int64)
    if fault == "row4_as_3":
        r = np.where(r == 4, 3, r)
    if fault == "other_view":
        view = other
    if fault == "assume_contig" or view.n_inner == 0:
        return (0 if fault in ("drop_offset", "assume_contig") else view.offset) + r * cols
    off, n, so, si = view
    if fault == "swap_strides":
        so, si = si, so
    if fault == "n_inner_plus":
        n += 1
    if fault == "n_inner_minus":
        n -= 1
    if fault == "drop_offset":
        off = 0
    q, m = (r % n, r // n) if fault == "swap_divmod" else (r // n, r % n)
    return off + q * so + m * si


def excused(fault, side, sname, dname):
    """-> the reason why the layout of `side` cannot hold the fault, or None"""
    name, other = (sname, dname) if side == "gather" else (dname, sname)
    if fault == "store_past_cols":
        return "a load re-reads the row's last vector by design: only a store past cols is a fault" if side == "gather" else None
    if fault == "other_view":
        return "both tensors have the same view" if name == other else None
    if fault == "row4_as_3":
        return "every row of an expanded tensor is the same memory" if name == "expanded" else None
    if name == "contig":
        return "a contiguous tensor has no offset, no strides and no n_inner to get wrong"
    if fault == "assume_contig":
        return None
    if name == "expanded" and fault != "drop_offset":
        return "both strides of an expanded tensor are 0, so every row is the same memory however r is split"
    if fault == "drop_offset" and name in ("every_other", "transposed"):
        return "the layout's offset is 0"
    if fault == "n_inner_plus" and name in V.LAYOUTS_2D:
        return "a 2-D view has n_inner = rows: with n_inner + 1 the quotient stays 0 and the remainder stays r (n_inner - 1 is seen)"
    return None


def restated_launch(data, sv, dv, dt, s_epv, d_epv, fault=None, side=None):
    """-> (buffer the launch leaves, buffer a correct launch leaves).  Both are large enough for every faulty address; what lies behind
    the real allocation reads as the hostile fill and is not compared (a faulty store there shows by the canaries of its due place)."""
    rows, cols = data.shape
    u = G.uint_of(dt)
    gs = faulty_starts(sv, dv, rows, cols, fault if side == "gather" else None)
    ss = faulty_starts(dv, sv, rows, cols, fault if side == "scatter" and fault != "store_past_cols" else None)
    src, _ = V.source_buffer(data, sv, dt)
    big = V.hostile(dt)[0]
    room = int(max(gs.max(), ss.max())) + cols + d_epv
    if room > src.size:
        src = np.concatenate([src, np.full(room - src.size, big, u)])
    x = np.stack([src[s: s + cols] for s in gs])
    want = V.scatter_expected(V.as_addressed(data, sv), dv, dt)
    got = np.full(max(room, want.size), V.CANARY[dt], u)
    for r, s in enumerate(ss):
        got[s: s + cols] = x[r]
    if fault == "store_past_cols" and side == "scatter":
        for r, s in enumerate(ss):
            got[s + cols: s + cols + d_epv] = x[r, -d_epv:]
    return got[: want.size], want


@pytest.mark.parametrize("form", V.FORMS)
def test_every_seeded_fault_is_seen_by_every_pairing_that_can_hold_it(form):
    done = set()
    holders = {(f, side): set() for f in FAULTS for side in ("gather", "scatter")}
    unseen = []
    for c in V.cases(form):
        cols = V.case_cols(c)
        names = c.pairing[1:]
        for i, (sv, dv, rows, se, de) in enumerate(views_of(c)):
            key = (cols, se, de, names[i], names[-1])
            if key in done:             # (the addressing depends on nothing else)
                continue
            done.add(key)
            dt = {8: "bf16", 4: "fp32"}[de]      # the restated launch moves rows unchanged: one element type, the destination's
            data = V.row_bits(dt, cols, rows)
            got, want = restated_launch(data, sv, dv, dt, se, de)
            assert np.array_equal(got, want), c
            for fault in FAULTS:
                for side in ("gather", "scatter"):
                    if excused(fault, side, names[i], names[-1]):
                        continue
                    holders[(fault, side)].add((names[i], names[-1]))
                    got, want = restated_launch(data, sv, dv, dt, se, de, fault, side)
                    if np.array_equal(got, want):
                        unseen.append((c.form, c.width, names[i], names[-1], fault, side))
    assert not unseen, (len(unseen), unseen[:8])
    for (fault, side), held in holders.items():
        if (fault, side) != ("store_past_cols", "gather"):
            assert held, (form, fault, side, "no pairing of this launch form can hold the fault")


def test_the_excuses_are_true():
    """an excused (fault, layout) leaves every address as it was -- that is why it cannot be seen, and the only reason accepted -- except
    the load's re-read of the last vector, which is the design"""
    cols, n = 56, 0
    for sname, dname in [(s, d) for _, s, d in V.PAIRINGS] + [(t[1], t[3]) for t in V.TRIPLES] + [(t[2], t[3]) for t in V.TRIPLES]:
        rows = max(V.rows_of(sname), V.rows_of(dname))
        sv, dv = V.layout(sname, cols, 8, rows), V.layout(dname, cols, 8, rows)
        for fault in FAULTS:
            for side, v, o in (("gather", sv, dv), ("scatter", dv, sv)):
                if excused(fault, side, sname, dname) and fault != "store_past_cols":
                    n += 1
                    assert np.array_equal(faulty_starts(v, o, rows, cols, fault), V.row_starts(v, rows, cols)), (fault, side, sname, dname)
    assert n > 20
