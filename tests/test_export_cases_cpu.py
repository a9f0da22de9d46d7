"""CPU tier of the export kernels' launch-shape tests: the ladder, the shapes and the inputs of tests/export_cases.py are worth running.
Structure (every rung of by_reg_shape, which launch_export_reg follows, with its two widths, rows of every mode in one launch, edge bins, fractions either side of
cmax + 0.5, exact ties, the int4 packer's nibble pairs, what fp16 cannot hold), the restatement pre_round -> round -> clamp -> pack -> count
against the oracle on every case, and SEEDED FAULTS in that restatement: each must change a compared output (packed bytes or overflow
counts) on EVERY case that holds what the fault touches, and the set of such cases is non-empty per dtype and per kernel body.  No kernel
runs.

One fault of the list cannot be seeded: moving the mode-1 / mode-2 threshold.  Mode 2 (element-wise saturation) is right for every row,
and mode 1 (the clamp behind the magic-constant add) is right for every row without a NaN bin, whatever its top bin; a row with a NaN bin
has a NaN or infinite top bin, which no finite threshold admits to mode 1.  test_the_threshold_position_is_not_observable asserts exactly
that on every finite row whose top bin is 2^21 or more, with the mode-1 arithmetic restated in float32.

Measured: 25 tests in about 60 s on one CPU core; the three per-case tests of a dtype and kind share ONE walk over its cases (survey)."""
import os
import re

import numpy as np
import pytest

import export_cases as E
from export_cases import CBITS, EPV, RUNGS

DTYPES = ["bf16", "fp16", "fp32"]
KINDS = ["sym", "asym"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32MIN, I32MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def idx_code(q):
    """rounded pre-round values -> the oracle's int32 coding of a bin (NaN -> INT32_MIN, +-Inf -> +-INT32_MAX, beyond 2e9 -> +-2e9)"""
    q = np.asarray(q, np.float64)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(q), I32MIN, np.where(np.isinf(q), np.sign(q) * I32MAX, np.clip(q, -2.0e9, 2.0e9)))
    return out.astype(np.int64)


class Ctx:
    """everything the assertions need of one case"""

    def __init__(self, dt, c, sh):
        self.dt, self.c, self.sh = dt, c, sh
        self.x = E.export_inputs(dt, *c, sh.cols, sh.rows)
        self.plants, self.names = E.export_plants(dt, *c, sh.cols, sh.rows)
        self.bytes, self.scales, self.over = E.expected(dt, *c, sh.cols, sh.rows)
        self.p = E.pre_round(self.x, dt, c.kind, c.bits, c.autocast, self.scales).astype(np.float64)
        self.cmin, self.cmax = E.crange(c)
        self.ints, self.bad = E.restate(self.p, self.cmin, self.cmax)
        self.top, self.mode = E.row_modes(self.x, dt, c, self.scales)
        self.tag = f"{dt} {c} {sh}"

    def changed(self, ints=None, bad=None, packed=None):
        """a faulty restatement differs from the expected output in a compared array"""
        if packed is None:
            packed = E.pack(self.ints if ints is None else ints, self.c.container)
        over = (self.bad if bad is None else bad).sum(1)
        return bool((packed != self.bytes).any() or (over != self.over).any())


def walk(dt, kind):
    for c, sh in E.cross(dt, kind):
        yield Ctx(dt, c, sh)


def on_grid(v, dt, c):
    """v is a value of the arithmetic torch.round's operand is computed in (fp32 under autocast and for fp32 tensors)"""
    sig = 24 if (dt == "fp32" or c.autocast) else E.SIG[dt]
    if dt == "fp16" and sig != 24 and abs(v) >= 65520:
        return False
    m = abs(int(v))
    return m == 0 or (m >> max(0, m.bit_length() - sig)) << max(0, m.bit_length() - sig) == m


def ulp_at(v, dt, c):
    sig = 24 if (dt == "fp32" or c.autocast) else E.SIG[dt]
    return 2.0 ** (int(np.floor(np.log2(abs(v)))) - (sig - 1))


_reach = {}


def reachable(k, r, b, key=None):
    """exhaustively: some finite 16-bit pattern between row r's extremes has the unclamped bin b (or a pre-round value that b(), named by
    key, accepts).  Rows of many cases share their scales and extremes, so the answers are kept."""
    xr = E.to_f32(k.x[r], k.dt).numpy().astype(np.float64)
    lo, hi = float(np.nanmin(xr)), float(np.nanmax(xr))
    ck = (k.dt, k.c.kind, k.c.bits, k.c.autocast, k.scales[r].tobytes(), lo, hi, key if callable(b) else ("bin", int(b)))
    if ck not in _reach:
        allp = np.arange(65536, dtype=np.uint16)
        v = E.to_f32(allp, k.dt).numpy().astype(np.float64)
        ok = np.isfinite(v) & (v >= lo) & (v <= hi)
        p = E.pre_round(allp[None, :], k.dt, k.c.kind, k.c.bits, k.c.autocast, k.scales[r:r + 1])[0].astype(np.float64)
        with np.errstate(invalid="ignore"):
            _reach[ck] = bool((ok & (b(p) if callable(b) else (np.rint(p) == b))).any())
    return _reach[ck]


# ---- the ladder and the case list ----------------------------------------------------------------------------------------------------------

def test_the_ladder_restates_launch_export_reg():
    """launch_export_reg takes its launch shape from by_reg_shape (fq_shapes.h) and from nowhere else; that RUNGS says what by_reg_shape
    says, for every nvec, is asserted against the compiled header in tests/test_shape_tables_cpu.py"""
    src = open(os.path.join(ROOT, "llm-qat_amd", "csrc", "fq_export.hip")).read()
    body = src[src.index("void launch_export_reg"):src.index("int export_t(")]
    flat = re.sub(r"\s+", " ", body)
    assert "by_reg_shape(nvec, [&](auto tpr, auto vpt) {" in flat and "launch_rows<TPR>(row_export_kernel<DT, TPR, VPT, ASYM, NTL>, a.rows, st, a);" in flat
    assert "switch" not in body and "#define" not in body and src.count("row_export_kernel<") == 1
    assert len(RUNGS) == 18 and RUNGS[0].lo == 0 and RUNGS[-1].hi == E.REG_MAX_VEC == 8192
    for a, b in zip(RUNGS, RUNGS[1:]):
        assert a.hi == b.lo
    brackets = {64: 192, 128: 384, 256: 768, 512: 4096, 1024: 8192}
    for r in RUNGS:
        assert r.hi == r.tpr * r.vpt and r.lo in (r.tpr * (r.vpt - 1), {64: 0, 128: 192, 256: 384, 512: 768, 1024: 4096}[r.tpr])
        assert r.hi <= brackets[r.tpr] and r.slots == {5: 6, 7: 8}.get(r.vpt, r.vpt) and r.tpr * r.slots >= r.hi
        for nvec in (r.lo + 1, r.hi):
            assert (nvec + r.tpr - 1) // r.tpr == r.vpt
    assert sorted((r.tpr, r.vpt) for r in RUNGS) == sorted([(64, 1), (64, 2), (64, 3), (128, 2), (128, 3), (256, 2), (256, 3)] +
                                                           [(512, v) for v in range(2, 9)] + [(1024, v) for v in range(5, 9)])


@pytest.mark.parametrize("dt", DTYPES)
def test_every_rung_has_its_two_widths_and_the_cross_its_launch_count(dt):
    epv = EPV[dt]
    shapes = E.widths(dt)
    for i, r in enumerate(RUNGS):
        mine = [s for s in shapes if s.rung == i]
        assert {(s.kind, s.nvec) for s in mine if s.rows == 5} == {("dup", r.hi - 1), ("tail", r.lo + 1)}
        assert {s.rows for s in mine} == ({1, 3, 4, 5} if r.tpr == 64 else {5})
        for s in mine:
            assert E.rung_of(s.nvec) == i and s.cols == s.nvec * epv and r.tpr * r.slots > s.nvec        # at least one empty slot
            if s.kind == "tail" and r.lo == r.tpr * (r.vpt - 1):
                assert s.nvec - r.lo == 1                          # the last slot-set holds one vector (the first rung of a thread count
                #                                                    starts where the narrower kernel ends, not on a multiple of its own)
    assert max(s.rows * s.cols for s in shapes) <= 5 * 65536 and len(shapes) == 54
    assert len(E.cross(dt)) == {"bf16": 1188, "fp32": 720, "fp16": 900}[dt]
    assert len(E.combos(dt)) == (18 if dt == "fp32" else 22)
    bodies = {E.body_of(c) for c in E.combos(dt)}
    assert bodies == {"int4", "int8", "general", "asym"}
    for c in E.combos(dt):      # each body x container x the modes it can meet: a saturating combination per body and container that has one
        assert c.autocast is False or c.kind == "sym"
    assert {(E.body_of(c), c.container) for c in E.combos(dt) if E.saturating(c)} >= {("int4", "int4"), ("int8", "int8"), ("general", "int16"),
                                                                                      ("asym", "int4"), ("asym", "int8"), ("asym", "int16")}


# ---- the restatement and the structure, per case ---------------------------------------------------------------------------------------------

def tie_up(v):
    return (np.abs(v - np.trunc(v)) == 0.5) & (np.rint(v) > v)


def tie_down(v):
    return (np.abs(v - np.trunc(v)) == 0.5) & (np.rint(v) < v)


def check_structure(k, st):
    """one case: the restatement equals the oracle, and the case holds what export_inputs promises"""
    dt = k.dt
    epv = EPV[dt]
    sign = int(E.SIGN[dt])
    for _ in (0,):
        c, sh, x, p = k.c, k.sh, k.x, k.p
        tag = k.tag
        # rint(pre_round) is the oracle's unclamped bin; round -> clamp -> pack -> count is the oracle's export
        idx = E.unclamped(dt, c.kind, c.bits, c.autocast, x)
        assert np.array_equal(idx_code(np.rint(p)), idx.astype(np.int64)), tag
        assert np.array_equal(E.pack(k.ints, c.container), k.bytes) and np.array_equal(k.bad.sum(1), k.over), tag
        finite_kind = np.array([n in ("mid", "mid2", "pow2", "tiny") for n in k.names])
        lastvec = (sh.nvec - 1) * epv

        # -- modes
        modes = set(k.mode.tolist())
        plain16 = dt == "fp16" and not c.autocast
        if E.saturating(c) and sh.rows >= 3:
            if dt != "fp16":           # (below 5 rows a width of 22 bits or more has no mode-1 row: that is `mid`, the last one)
                assert modes == ({0, 2} if (E.hi_bits(c) and sh.rows < 5) else {0, 1, 2}), (tag, k.mode, k.top)
            elif plain16:                       # the module text: no mode-0 row; mode 1 while the full-scale bin is finite in fp16; the s = Inf
                full = 2 ** c.bits - 1 if c.kind == "asym" else 2 ** (c.bits - 1) - 1       # row and the row of zeros
                assert 0 not in modes and 2 in modes and ((1 in modes) == (full < 65520)), (tag, k.mode, k.top)
                if c.kind == "sym":
                    r = k.names.index("sinf")
                    assert np.isinf(k.scales[r, 0]) and k.over[r] == sh.cols and not np.isfinite(p[r]).any(), tag
                    if c.bits > 16:
                        ok = finite_kind & np.isfinite(k.scales[:, 0])
                        assert ok[finite_kind].all() and (E.row_bounds(x, dt, False)[finite_kind, 0] >= (2.0 ** (c.bits - 1) - 1) / 65504).all(), tag
                if sh.rows >= 4:
                    assert k.over[3] == sh.cols, tag           # 0 * Inf, 0 / 0
            else:
                assert {1, 2} <= modes and ((0 in modes) == (sh.rows >= 4)), (tag, k.mode)       # mode 0: the row of zeros
        if not E.saturating(c):      # a fitting width: mode 0, or (16-bit arithmetic rounding s or the product up) a top bin of cmax + 1
            fin = finite_kind & np.isfinite(k.top)
            assert (k.top[fin] <= k.cmax + 1).all() and ((k.mode[fin] == 0).all() or (dt != "fp32" and not c.autocast)), (tag, k.mode, k.top)
        if dt == "bf16" and c == E.Combo("sym", 8, "int8", False) and sh.rows == 5:
            assert k.top[4] == 128 and k.mode[4] == 1 and k.top[0] == 127 and k.mode[0] == 0, (tag, k.top)     # mode 1 next to mode 0
            st["tops128"] += 1

        # -- rows by name
        for r, n in enumerate(k.names):
            row = x[r]
            if n == "zero":
                assert ((row & (sign - 1)) == 0).all() and ((row & sign) != 0).sum() == 1, tag
            elif n == "special" and sh.cols > 1:
                v = E.to_f32(row, dt).numpy()
                assert np.isnan(v).sum() + np.isinf(v).sum() == 1 and k.mode[r] == 2, tag
                st["specials"].setdefault((sh.rung, sh.rows), set()).add("nan" if np.isnan(v).any() else "pinf")
                if np.isnan(v).any():
                    assert k.over[r] == sh.cols, tag       # a NaN scale: every bin NaN, every element counted
            if r == 0 and sh.nvec >= 2:
                assert (row == sign).any(), tag            # a -0.0
            elif n == "tiny" and E.saturating(c):
                assert k.mode[r] == 0 and k.over[r] == 0 and abs(k.top[r]) >= 2, (tag, k.top)

        # -- edge bins, fractions and ties inside every mode-1 / mode-2 row with a finite scale
        if sh.nvec < 2:
            continue                                       # (one vector: room for the extremes and a few edges only)
        q = np.rint(p)
        by_row = {}
        for pl in k.plants:
            by_row.setdefault(pl.row, []).append(pl)
        for r in np.flatnonzero(finite_kind & (k.mode > 0)):
            mine = by_row.get(r, [])
            lo_reach = -k.top[r] if c.kind == "sym" else 0
            for b in (k.cmax + 1, k.cmin - 1, k.cmax, k.cmin):
                here = [pl for pl in mine if pl.what == "bin" and pl.arg == b and q[r, pl.col] == b]
                if lo_reach <= b <= k.top[r] and on_grid(b, dt, c):
                    if not here and dt != "fp32":      # a 16-bit input grid can step over a bin: then NO pattern between the row's extremes
                        assert not reachable(k, r, b), (tag, r, b, "reachable, yet not planted")          # gives it (all 65536 tried)
                        continue
                    assert here, (tag, r, b, k.top[r])
                    if b == k.cmax + 1:
                        assert any(pl.col >= lastvec for pl in here), (tag, r, "cmax + 1 belongs in the last vector")
                elif lo_reach <= b <= k.top[r]:
                    assert not (q[r] == b).any(), (tag, r, b, "off the grid, yet present")      # the exemption, asserted
            edges = [pl for pl in mine if pl.what in ("bin", "frac_lo", "frac_hi")]
            assert any(pl.col >= lastvec and k.bad[r, pl.col] for pl in mine), (tag, r, "an overflowing element belongs in the last vector")
            assert not edges or any(pl.col < epv for pl in edges), (tag, r, "an edge element belongs in vector 0")
            if k.top[r] >= k.cmax + 1:
                f_lo = (p[r] > k.cmax) & (p[r] < k.cmax + 0.5)
                f_hi = (p[r] > k.cmax + 0.5) & (p[r] < k.cmax + 1)
                if ulp_at(k.cmax, dt, c) <= 0.125:
                    for what, f, inside in (("frac_lo", f_lo, lambda v: (v > k.cmax) & (v < k.cmax + 0.5)),
                                            ("frac_hi", f_hi, lambda v: (v > k.cmax + 0.5) & (v < k.cmax + 1))):
                        if not any(pl.what == what and f[pl.col] for pl in mine):
                            assert dt != "fp32" and not reachable(k, r, inside, (what, k.cmax)), (tag, r, what)     # (all 65536 patterns tried)
                elif ulp_at(k.cmax, dt, c) >= 0.5:
                    assert not f_lo.any() and not f_hi.any(), (tag, r)                           # the grid has none: asserted, not assumed
        frac = np.abs(p - np.trunc(p)) == 0.5
        for pl in k.plants:
            if pl.what == "tie":
                assert p[pl.row, pl.col] == pl.arg and frac[pl.row, pl.col], (tag, pl)
        # at least one exact tie that rounds up and one that rounds down, per case; where a case has none, no 16-bit pattern between the
        # extremes of any of its finite-scale rows gives one (all 65536 tried per row) -- fp32 tensors always have both
        fin_rows = np.flatnonzero(finite_kind & np.isfinite(k.scales[:, 0]) & (k.scales[:, 0] != 0))
        with np.errstate(invalid="ignore"):
            for name, pred in (("up", tie_up), ("down", tie_down)):
                if pred(p).any():
                    st["ties"][name] += 1
                    continue
                assert dt != "fp32", (tag, "no tie that rounds", name)
                for r in fin_rows:
                    assert not reachable(k, r, pred, "tie " + name), (tag, r, "a tie that rounds " + name + " exists on the grid, yet none is planted")
                st["no_tie"][name].add(c)
        if True:
            r = k.names.index("pow2")
            halves = [pl for pl in k.plants if pl.what == "half"]
            full = 2 ** c.bits - 1 if c.kind == "asym" else 2 ** (c.bits - 1) - 1
            if on_grid(full, dt, c) and not (dt == "fp16" and not c.autocast and full > 2047):
                got = sorted(p[pl.row, pl.col] for pl in halves)
                assert got == ([full / 2] if c.kind == "asym" else [-full / 2, full / 2]), (tag, got)
                if c.kind == "sym":            # at least one tie that rounds up and one that rounds down
                    assert (frac[r] & (q[r] > p[r])).any() and (frac[r] & (q[r] < p[r])).any(), tag
            else:
                assert not any(frac[pl.row, pl.col] for pl in halves) or not np.isfinite(k.scales[r, 0]), (tag, "qmax / 2 is off the grid")
        with np.errstate(invalid="ignore"):
            if (frac & (np.abs(q) < np.abs(p)) & (np.abs(q) < k.cmax)).any():
                st["even_ties"].add(E.body_of(c))


_surveys = {}


def survey(dt, kind):
    """ONE walk over the cross of (dt, kind) for the three per-case tests below: each case is built, sent through the oracle and restated
    once; the first failed assertion of each checker is kept for its test"""
    if (dt, kind) not in _surveys:
        st = {"err": {}, "tops128": 0, "specials": {}, "even_ties": set(), "ties": {"up": 0, "down": 0}, "no_tie": {"up": set(), "down": set()},
              "undetected": [], "held": {f: set() for f in FAULTS}, "big_rows": 0, "nan_rows": 0, "cases": 0}
        for k in walk(dt, kind):
            st["cases"] += 1
            for name, fn in (("structure", check_structure), ("faults", check_faults), ("threshold", check_threshold)):
                if name not in st["err"]:
                    try:
                        fn(k, st)
                    except AssertionError as e:
                        st["err"][name] = e
        _surveys[(dt, kind)] = st
    return _surveys[(dt, kind)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_the_oracle_and_every_case_holds_what_it_should(dt, kind):
    st = survey(dt, kind)
    if "structure" in st["err"]:
        raise st["err"]["structure"]
    assert st["cases"] == len(E.cross(dt, kind))
    for i in range(len(RUNGS)):        # a NaN row and a +Inf row at EVERY rung (one per width), and at 3 and 4 rows where the rung has them
        for rows in ((5, 3, 4) if RUNGS[i].tpr == 64 else (5,)):
            assert st["specials"].get((i, rows)) == {"nan", "pinf"}, (i, rows, st["specials"].get((i, rows)))
    assert st["even_ties"] == {E.body_of(c) for c in E.combos(dt, kind)}, st["even_ties"]       # ties that half-to-even rounds TOWARDS zero, per body
    assert st["ties"]["up"] > 0 and st["ties"]["down"] > 0
    print(dt, kind, "cases with a tie up / down:", st["ties"], "of", st["cases"], "| combinations with a case that provably has none:",
          {n: sorted(set((c.bits, c.container, c.autocast) for c in v)) for n, v in st["no_tie"].items()})
    if dt == "fp32":
        assert not st["no_tie"]["up"] and not st["no_tie"]["down"]
    if dt == "bf16" and kind == "sym":
        assert st["tops128"] == 18 * 2


@pytest.mark.parametrize("dt", DTYPES)
def test_int4_nibble_pairs_sit_at_every_byte_position_of_a_lane(dt):
    """(-8, +7), (+7, -8), (-1, 0), (0, -1) for Sym and (15, 0), (0, 15) for Asym in the EXPECTED bytes, at each of the EPV / 2 byte positions
    of a lane's packed word, counted over the cases of a dtype"""
    nb = EPV[dt] // 2
    want = {"sym": {0x78, 0x87, 0x0F, 0xF0}, "asym": {0x0F, 0xF0}}
    seen = {(kind, v): set() for kind in KINDS for v in want[kind]}
    for c, sh in E.cross(dt):
        if c.container != "int4":
            continue
        by = E.expected(dt, *c, sh.cols, sh.rows)[0]
        pos = np.arange(by.shape[1]) % nb
        for v in want[c.kind]:
            seen[(c.kind, v)] |= set(pos[(by == v).any(0)].tolist())
    for key, s in seen.items():
        assert s == set(range(nb)), (key, s)


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------------------

def mode1_arith(p, c):
    """the kernel's mode-1 arithmetic restated in float32: p + 1.5 * 2^23 (+ 8 for Sym int4), clamp, count what the clamp moved, low bits"""
    cmin, cmax = E.crange(c)
    ib = 8 if (c.container == "int4" and c.kind == "sym") else 0
    magic = np.float32(12582912.0 + ib)
    f = (np.asarray(p, np.float32) + magic).astype(np.float32)
    cl = np.clip(f, np.float32(magic + cmin), np.float32(magic + cmax))
    low = cl.view(np.uint32).astype(np.int64) - 0x4B400000 - ib
    return low, cl != f


def wrap(q, c):
    """mode 0 on a bin that does not fit: the low container bits of the two's complement integer"""
    cb = CBITS[c.container]
    with np.errstate(invalid="ignore"):
        v = np.where(np.isfinite(q), np.clip(q, -2.0 ** 22, 2.0 ** 22), 0).astype(np.int64) & ((1 << cb) - 1)
    return v if c.kind == "asym" else np.where(v >= 1 << (cb - 1), v - (1 << cb), v)


FAULTS = ("ties_away", "clamp_then_round", "count_truncated", "cmin_counted", "cmax1_not_counted", "nan_stored", "nan_not_counted",
          "nibbles_swapped", "offset_binary", "nibble_borrow", "duplicates_counted", "previous_rows_mode", "row4_row3_scales",
          "asym_int16_signed")
# a fault that only some combinations can hold: the three nibble faults need an int4 container (offset binary and the borrow: Sym only),
# the signed 16-bit range needs Asym into int16
ONLY = {"nibbles_swapped": lambda c: c.container == "int4", "offset_binary": lambda c: c.container == "int4" and c.kind == "sym",
        "nibble_borrow": lambda c: c.container == "int4" and c.kind == "sym", "asym_int16_signed": lambda c: c.kind == "asym" and c.container == "int16"}


def seeded(k, name):
    """-> None if the case holds nothing the fault touches, else True / False: the faulty restatement changed a compared output"""
    c, p, sh = k.c, k.p, k.sh
    q = np.rint(p)
    nan = np.isnan(p)
    cmin, cmax = k.cmin, k.cmax
    with np.errstate(invalid="ignore"):
        if name == "ties_away":
            touch = (np.abs(p - np.trunc(p)) == 0.5) & (np.abs(q) < np.abs(p)) & (np.abs(q) < cmax)
            if not touch.any():
                return None
            ints, bad = E.restate(np.where(touch, np.sign(p) * np.floor(np.abs(p) + 0.5), q), cmin, cmax)
            return k.changed(ints, bad)
        if name == "clamp_then_round":        # the clamp before the rounding, counting what it moved: 7.3 is counted
            touch = ((p > cmax) & (p < cmax + 0.5)) | ((p < cmin) & (p > cmin - 0.5))
            return k.changed(bad=k.bad | touch) if touch.any() else None
        if name == "count_truncated":         # the 7.6 element kept as 7 and not counted
            touch = ((p > cmax + 0.5) & (p < cmax + 1)) | ((p < cmin - 0.5) & (p > cmin - 1))
            return k.changed(bad=k.bad & ~touch) if touch.any() else None
        if name == "cmin_counted":
            touch = q == cmin
            return k.changed(bad=k.bad | touch) if touch.any() else None
        if name == "cmax1_not_counted":
            touch = q == cmax + 1
            return k.changed(bad=k.bad & ~touch) if touch.any() else None
        if name == "nan_stored":
            return k.changed(ints=np.where(nan, cmax, k.ints)) if nan.any() else None
        if name == "nan_not_counted":
            return k.changed(bad=k.bad & ~nan) if nan.any() else None
        if name == "nibbles_swapped":
            if sh.cols < 8:
                return None
            return k.changed(packed=((k.bytes >> 4) | (k.bytes << 4)) & 0xFF)
        if name == "offset_binary":
            return k.changed(packed=k.bytes ^ 0x88)
        if name == "nibble_borrow":
            v = k.ints if sh.cols % 2 == 0 else np.concatenate([k.ints, np.zeros((sh.rows, 1), np.int64)], 1)
            if not (v[:, 0::2] < 0).any():
                return None
            return k.changed(packed=((v[:, 0::2] + (v[:, 1::2] << 4)) & 0xFF).astype(np.uint8))
        if name == "duplicates_counted":      # the row's last vector counted once more per slot at or beyond nvec
            r = RUNGS[sh.rung]
            epv = EPV[k.dt]
            last = k.bad[:, (sh.nvec - 1) * epv:sh.nvec * epv].sum(1) * (k.mode > 0)
            if not last.any():
                return None
            return bool(((k.bad.sum(1) + last * (r.tpr * r.slots - sh.nvec)) != k.over).any())
        if name == "previous_rows_mode":      # mode 0 (no clamp, no count) on a row behind a mode-0 row
            rows = [r for r in range(1, sh.rows) if k.mode[r - 1] == 0 and k.mode[r] > 0]
            if not rows:
                return None
            ints, bad = k.ints.copy(), k.bad.copy()
            for r in rows:
                ints[r], bad[r] = wrap(q[r], c), False
            return k.changed(ints, bad)
        if name == "row4_row3_scales":
            if sh.rows < 5 or sh.nvec < 2:      # (one vector: at 31 bits its few elements saturate under either scale)
                return None
            sc = k.scales.copy()
            if sc[4].tobytes() == sc[3].tobytes():      # (from 22 bits on `+ 1e-6` rules both the zero row's scale and the small `mid` row's:
                return None                             # in bf16 the two can be the same number, and the fault then touches nothing)
            sc[4] = sc[3]
            ints, bad = E.restate(E.pre_round(k.x, k.dt, c.kind, c.bits, c.autocast, sc), cmin, cmax)
            return k.changed(ints, bad)
        if name == "asym_int16_signed":       # bins 32768 .. 65535 taken for negative numbers
            if not (q >= 32768).any():
                return None
            ints, bad = E.restate(p, -32768, 32767)
            return k.changed(ints, bad)
    raise KeyError(name)


def check_faults(k, st):
    for f in FAULTS:
        if f in ONLY and not ONLY[f](k.c):
            continue
        res = seeded(k, f)
        if res is None:
            continue
        st["held"][f].add(E.body_of(k.c))
        if not res:
            st["undetected"].append((f, k.tag))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_seeded_fault_changes_a_compared_output(dt, kind):
    st = survey(dt, kind)
    if "faults" in st["err"]:
        raise st["err"]["faults"]
    undetected, held = st["undetected"], st["held"]
    assert not undetected, (len(undetected), undetected[:10])
    for f in FAULTS:        # the set of cases that hold what the fault touches is non-empty for every body the fault can live in
        bodies = {E.body_of(c) for c in E.combos(dt, kind) if f not in ONLY or ONLY[f](c)}
        if f in ("clamp_then_round", "count_truncated", "cmax1_not_counted", "duplicates_counted", "previous_rows_mode"):
            bodies = {E.body_of(c) for c in E.combos(dt, kind) if E.saturating(c) or (dt == "bf16" and c == E.Combo("sym", 8, "int8", False))}
        if f in ("clamp_then_round", "count_truncated"):      # only where the arithmetic's grid has values between cmax and cmax + 1: bf16
            bodies = {E.body_of(c) for c in E.combos(dt, kind) if E.saturating(c) and ulp_at(E.crange(c)[1], dt, c) <= 0.125}   # has none at 127
        assert held[f] >= bodies, (f, held[f], bodies)


def check_threshold(k, st):
    c, sh = k.c, k.sh
    if c.bits < 22:
        return
    low, moved = mode1_arith(k.p, c)
    for r in range(sh.rows):
        if np.isnan(k.p[r]).any():
            assert not (k.top[r] < np.inf), (k.tag, r, k.top[r])
            st["nan_rows"] += 1
            continue
        if k.top[r] >= 2.0 ** 21:
            st["big_rows"] += 1
            assert np.array_equal(low[r], k.ints[r]) and np.array_equal(moved[r], k.bad[r]), (k.tag, r)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_threshold_position_is_not_observable(dt, kind):
    """what mode 1 computes on rows whose top bin is 2^21 or more (a threshold at 2^23 or beyond would send them there) equals the expected
    output wherever the row holds no NaN bin -- and every row that holds one has a NaN or infinite top bin, so no threshold sends it there;
    the same arithmetic DOES differ on a NaN bin, which is what the threshold is for"""
    st = survey(dt, kind)
    if "threshold" in st["err"]:
        raise st["err"]["threshold"]
    assert st["big_rows"] > 0 and st["nan_rows"] > 0
