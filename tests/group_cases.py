"""Shapes and inputs of the group-wise kernel's launch-shape tests, shared by the CPU tier (tests/test_group_cases_cpu.py, which proves
them sensitive against deliberately wrong reductions) and the GPU tier (tests/test_gpu_group_shapes.py, which runs fq_group_fwd on them).
numpy only, no product code.

A row of `cols` elements is nvec = cols / EPV 16-byte vectors; a group of g elements is gv = g / EPV of them.  The kernel picks one of ten
(threads per row, vectors per thread) instantiations from nvec, reduces each group inside an aligned gv-lane segment of a wave, and lets
out-of-range slots of the last sweep re-load the row's last vector."""
from collections import namedtuple

import numpy as np

from mx_reference import decode, encode

EPV = {"bf16": 8, "fp16": 8, "fp32": 4}
GVS = (4, 8, 16, 32, 64)          # vectors per group the validation of fq_group_fwd accepts
# mirrors by_group_shape (llm-qat_amd/csrc/fq_shapes.h; tests/test_shape_tables_cpu.py compares the two): lo < nvec <= hi runs group_reg_kernel<TPR, VPT>
Bracket = namedtuple("Bracket", "lo hi tpr vpt")
BRACKETS = [Bracket(0, 64, 64, 1), Bracket(64, 128, 64, 2), Bracket(128, 256, 128, 2), Bracket(256, 512, 256, 2), Bracket(512, 768, 256, 3),
            Bracket(768, 1024, 512, 2), Bracket(1024, 1536, 512, 3), Bracket(1536, 2048, 512, 4), Bracket(2048, 4096, 1024, 4),
            Bracket(4096, 8192, 1024, 8)]

Case = namedtuple("Case", "bracket gv kind nvec rows cols g tpr vpt seed")


def bracket_of(nvec):
    return next(i for i, b in enumerate(BRACKETS) if b.lo < nvec <= b.hi)


def row_lengths(bi, gv):
    """-> {kind: nvec} of bracket bi for groups of gv vectors: "full" (the bracket's largest nvec: every slot in range), "tail" (the
    smallest multiple of gv above the lower bound: nearly every slot of the last sweep is out of range) and "mid" (a multiple of gv in
    between that is a multiple of neither 64 nor TPR).  A bracket that holds fewer than three multiples of gv (gv = 32 and 64 in the two
    64-wide brackets, gv = 64 in (128, 256]) yields the ones it has; multiples of gv = 64 are multiples of 64, so their "mid" only avoids
    TPR, which every bracket with TPR > 64 allows."""
    b = BRACKETS[bi]
    out = {"full": b.hi}
    tail = b.lo + gv
    if tail < b.hi:
        out["tail"] = tail
    cand = [n for n in range(tail + gv, b.hi, gv) if n % b.tpr and (n % 64 or gv == 64)]
    if cand:
        out["mid"] = min(cand, key=lambda n: (abs(n - (b.lo + b.hi) // 2), n))
    return out


def case_list(dtype):
    """every bracket x every served gv x {full, tail, mid} at 5 rows (not a multiple of the four rows a TPR == 64 workgroup holds), plus
    rows 1, 3 and 4 on a tail and a full row of each TPR == 64 bracket"""
    epv = EPV[dtype]
    out = []

    def add(bi, gv, kind, nvec, rows):
        b = BRACKETS[bi]
        out.append(Case(bi, gv, kind, nvec, rows, nvec * epv, gv * epv, b.tpr, b.vpt, len(out)))

    for bi in range(len(BRACKETS)):
        for gv in GVS:
            for kind, nvec in row_lengths(bi, gv).items():
                add(bi, gv, kind, nvec, 5)
    for bi, b in enumerate(BRACKETS):
        if b.tpr == 64:
            for rows in (1, 3, 4):
                add(bi, 4, "tail", row_lengths(bi, 4)["tail"], rows)
                add(bi, 16, "full", b.hi, rows)
    return out


def train_cases(dtype):
    """training mode: every bracket on the full and the tail length, the smallest and the largest gv, rows 5 and 3"""
    epv = EPV[dtype]
    out = []
    for bi, b in enumerate(BRACKETS):
        for gv in (4, 64):
            lens = row_lengths(bi, gv)
            for kind in ("full", "tail"):
                for rows in (5, 3):
                    if kind in lens:
                        out.append(Case(bi, gv, kind, lens[kind], rows, lens[kind] * epv, gv * epv, b.tpr, b.vpt, 1000 + len(out)))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

NAN = {"bf16": 0x7FC1, "fp16": 0x7E01, "fp32": 0x7FC00001}
PINF = {"bf16": 0x7F80, "fp16": 0x7C00, "fp32": 0x7F800000}
MAXFIN = {"bf16": 0x7F7F, "fp16": 0x7BFF, "fp32": 0x7F7FFFFF}
SIGN = {"bf16": 0x8000, "fp16": 0x8000, "fp32": 0x80000000}
TWO = {"bf16": 0x4000, "fp16": 0x4000, "fp32": 0x40000000}
# exponents e of a group's planted magnitude 1.5 * 2^e, three binades apart.  (Not lower: the quantizers add 1e-6 / 1e-8 to the extreme,
# and a group far below that quantizes to zeros whatever its maximum is -- it could not tell a wrong reduction from a right one.)
EXPS = {"bf16": np.arange(-9, 61, 3), "fp16": np.arange(-9, 16, 3), "fp32": np.arange(-9, 61, 3)}
EXPS_CLIP = np.arange(-9, 16, 3)                                                       # training mode: rows that reach +-2
EXPS_SAFE = np.arange(-12, -2, 3)                                                      # ... and rows that cannot
KINDS = ("nan", "pinf", "ninf", "zero", "maxfin", "subnormal", "allpos", "allneg", "const")
SAFE_KINDS = ("zero", "subnormal", "allpos", "allneg", "const")    # finite and below the clip wherever the group's magnitude is


def uint_of(dtype):
    return np.uint32 if dtype == "fp32" else np.uint16


def planted_positions(rows, ng, g, dtype, seed):
    """-> (pmax, pmin) int [rows, ng]: the element of group (r, j) that holds its largest magnitude, and the element that holds the
    extreme of the other sign.  EPV + 1 is odd and g a power of two, so the position walks through every element of every vector slot."""
    r, j = np.meshgrid(np.arange(rows), np.arange(ng), indexing="ij")
    pmax = (j * (EPV[dtype] + 1) + r * 3 + seed) % g
    return pmax, (pmax + g // 2) % g          # half a group away: another vector slot


def special_locations(nvec, gv):
    """group indices that carry special cases: the first and the last group of the row (the last is the neighbour of the duplicated tail)
    and the two groups on either side of the 16-lane and 32-lane boundaries (lanes 16, 32, 48 and the wave boundary) of the row's first and
    last wave, wherever such a boundary falls between two groups"""
    ng = nvec // gv
    loc = [0, ng - 1]
    last = (nvec - 1) // 64 * 64
    for base in sorted({0, last}):
        for b in (16, 32, 48, 64):
            v = base + b
            if 0 < v < nvec and v % gv == 0:
                loc += [v // gv - 1, v // gv]
    return sorted(set(loc))


def group_plan(rows, cols, g, dtype, seed, train=False):
    """-> kind [rows, ng] (object array of names: "normal", one of KINDS, "edge", "edge_nan") and e [rows, ng] (the group's exponent)"""
    epv = EPV[dtype]
    nvec, gv, ng = cols // epv, g // epv, cols // g
    kind = np.full((rows, ng), "normal", dtype=object)
    r, j = np.meshgrid(np.arange(rows), np.arange(ng), indexing="ij")
    if train:
        clip_row = (np.arange(rows) % 2 == 0)
        ec, es = EXPS_CLIP, EXPS_SAFE
        e = np.where(clip_row[:, None], ec[(11 * j + 4 * r + seed) % len(ec)], es[(3 * j + r + seed) % len(es)])
    else:
        ex = EXPS[dtype]
        e = ex[(11 * j + 4 * r + seed) % len(ex)]      # neighbours are 11 steps (fp16: 2 steps) or a wrap apart
    loc = special_locations(nvec, gv)
    free = [x for x in range(rows) if x not in (0, (len(loc) - 1) % rows)]
    if free and ng >= 2 and not train:
        # one row whose first and last group are plain, the first far above the last: a duplicated tail slot that read the row's FIRST
        # vector instead of its last would raise the last group's extremes
        rt = free[0]
        e[rt, 0] = max(x for x in ex if ng == 2 or x != e[rt, 1])
        e[rt, -1] = min(x for x in ex if ng == 2 or x != e[rt, -2])
    for li, gi in enumerate(loc):
        row = li % rows                                 # each location is special in one row: the other rows keep a plain group there
        names = KINDS
        if train and (row % 2 == 1 or row == 0):
            names = SAFE_KINDS
        kind[row, gi] = names[(li + seed) % len(names)]
    if train:
        for row in range(0, rows, 2):
            jc = (3 * row + seed) % ng
            want_nan = row == 2 or (rows < 3 and row == 0)
            if want_nan and ng > 1:
                kind[row, (jc + 1 + ng // 2) % ng if (jc + 1 + ng // 2) % ng != jc else (jc + 1) % ng] = "nan"
            kind[row, jc] = "edge_nan" if want_nan and ng == 1 else "edge"
            e[row, jc] = 3
    return kind, e


def group_inputs(rows, cols, g, dtype, seed, train=False):
    """bit patterns [rows, cols] (uint16, or uint32 for fp32).  Group j of a row is scaled by a power of two that depends on j (and on the
    row), its largest magnitude 1.5 * 2^e is ONE planted element, twice the planted element of the other sign and at least four times
    everything else, and the planted position walks with j and the row; the groups of special_locations() carry the special cases.
    train: even rows reach the clip +-2 (and hold a group with +-2 and the patterns one ulp on either side of them; row 2 -- row 0 where
    there is none -- also holds a NaN), odd rows stay below it."""
    epv = EPV[dtype]
    assert cols % g == 0 and g % epv == 0
    ng = cols // g
    u = uint_of(dtype)
    rng = np.random.default_rng(seed * 7919 + rows * 131 + ng)
    kind, e = group_plan(rows, cols, g, dtype, seed, train)
    pmax, pmin = planted_positions(rows, ng, g, dtype, seed)
    M = 1.5 * np.exp2(e.astype(np.float64))[:, :, None]
    fill = rng.uniform(1.0 / 16, 1.0 / 4, (rows, ng, g)) * np.where(rng.integers(0, 2, (rows, ng, g)) == 1, -1.0, 1.0)
    rr, jj = np.meshgrid(np.arange(rows), np.arange(ng), indexing="ij")
    sgn = np.where((rr + jj + seed) % 2 == 0, 1.0, -1.0)
    v = fill * M
    v[rr, jj, pmax] = sgn * M[:, :, 0]
    v[rr, jj, pmin] = -0.5 * sgn * M[:, :, 0]
    bits = encode(v.astype(np.float32).astype(np.float64), dtype).astype(u).reshape(rows, ng, g)
    sign, two = u(SIGN[dtype]), u(TWO[dtype])
    for r, j in zip(*np.nonzero(kind != "normal")):
        k = kind[r, j]
        b = bits[r, j]
        p, q = pmax[r, j], pmin[r, j]
        if k == "nan":
            b[p] = NAN[dtype] | (sign if (r + j) % 2 else 0)
        elif k == "pinf":
            b[p] = PINF[dtype]
        elif k == "ninf":
            b[p] = PINF[dtype] | sign
        elif k == "zero":
            b[:] = 0
            b[p] = sign
        elif k == "maxfin":
            b[p] = MAXFIN[dtype]
            b[q] = MAXFIN[dtype] | sign
        elif k == "subnormal":                      # mantissa-only patterns: the largest at p, its negative neighbour at q
            top = {"bf16": 0x7F, "fp16": 0x3FF, "fp32": 0x7FFFFF}[dtype]
            m = rng.integers(1, max(2, top // 2), g).astype(u)
            b[:] = m | np.where(rng.integers(0, 2, g) == 1, sign, u(0)).astype(u)
            b[p] = top
            b[q] = (top - 1) | sign
        elif k in ("allpos", "allneg"):
            b &= ~sign
            b[q] = encode(np.array([M[r, j, 0] / 32]), dtype).astype(u)[0]
            if k == "allneg":
                b |= sign
        elif k == "const":
            b[:] = b[p]
        elif k in ("edge", "edge_nan"):             # planted magnitude 12: +-2 and their neighbours are plain elements of the group
            edge = [two, two | sign, two + u(1), two - u(1), (two + u(1)) | sign, (two - u(1)) | sign]
            slots = [x for x in range(g) if x != p and x != q]
            for i, val in enumerate(edge):
                b[slots[(i * 5 + r) % len(slots)]] = val
            if k == "edge_nan":
                b[slots[(31 + r) % len(slots)]] = NAN[dtype]
    return bits.reshape(rows, cols)


def values(bits, dtype):
    """float64 values of bit patterns"""
    return decode(bits, dtype)


def oracle_view(bits, dtype):
    """what oracle.sym_fwd / asym_fwd take: uint16 bit patterns, float32 values for fp32"""
    return np.ascontiguousarray(bits).view(np.float32) if dtype == "fp32" else np.ascontiguousarray(bits)


def differs(a, b, dtype):
    """elementwise on bit patterns: the zero-tolerance comparison (any NaN equals any NaN) fails here"""
    e, m = {"bf16": (0x7F80, 0x7F), "fp16": (0x7C00, 0x3FF), "fp32": (0x7F800000, 0x7FFFFF)}[dtype]
    nan = lambda v: ((v & e) == e) & ((v & m) != 0)  # noqa: E731
    return (a != b) & ~(nan(a) & nan(b))


def reference(bits, g, dtype, kind, nbits=4, sem=0, autocast=False):
    """the CPU oracle (test infrastructure, independent of the kernels) on the [rows * cols / g, g] view -> bit patterns of bits' shape.
    sem: 0 = cpu_eager, 1 = device_eager; autocast: SymQuantizer's autocast arithmetic rounded once to the tensor dtype"""
    from oracle import oracle as O
    xv = oracle_view(bits.reshape(-1, g), dtype)
    if autocast:
        y = O.sym_fwd_autocast(xv, xv.shape[0], g, nbits, dtype, wide=False)[0]
    else:
        fn = O.sym_fwd if kind == "sym" else O.asym_fwd
        y = fn(xv, xv.shape[0], g, nbits, dtype, sem=sem, want_idx=False)[0]
    return y.view(uint_of(dtype)).reshape(bits.shape)


_inputs, _refs = {}, {}


def cached_inputs(dtype, c, train=False):
    """group_inputs of a Case, computed once per process and read-only"""
    key = (dtype, c, train)
    if key not in _inputs:
        _inputs[key] = group_inputs(c.rows, c.cols, c.g, dtype, c.seed, train)
        _inputs[key].flags.writeable = False
    return _inputs[key]


def cached_reference(dtype, c, kind, nbits=4, sem=0, autocast=False, train=False):
    key = (dtype, c, kind, nbits, sem, autocast, train)
    if key not in _refs:
        _refs[key] = reference(cached_inputs(dtype, c, train), c.g, dtype, kind, nbits, sem, autocast)
        _refs[key].flags.writeable = False
    return _refs[key]


def grad_bits(zeroed, dtype, seed):
    """a gradient of zeroed's shape whose NaN, +Inf, -Inf and -0.0 sit at positions the backward zeroes and at positions it keeps"""
    zeroed = np.asarray(zeroed, dtype=bool)
    u = uint_of(dtype)
    rng = np.random.default_rng(seed)
    b = encode(rng.standard_normal(zeroed.size).astype(np.float32).astype(np.float64), dtype).astype(u).reshape(-1)
    special = [NAN[dtype], PINF[dtype], PINF[dtype] | SIGN[dtype], SIGN[dtype]]
    flat = zeroed.reshape(-1)
    for sel in (np.flatnonzero(flat), np.flatnonzero(~flat)):
        if sel.size:
            pick = sel[rng.integers(0, sel.size, min(sel.size, 24))]
            for i, p in enumerate(pick):
                b[p] = special[i % 4]
    return b.reshape(zeroed.shape)


def clip_predicate(bits, dtype, lo=-2.0, hi=2.0):
    """the STE backward's predicate x >= hi or x <= lo (NaN compares false) -> bool"""
    v = values(bits, dtype)
    with np.errstate(invalid="ignore"):
        return (v >= hi) | (v <= lo)


def row_bounds(bits, dtype, asym):
    """float32 [rows, 2]: the row's max / -max of |x| (Sym) or max / min (Asym); NaN if the row holds one"""
    v = values(bits, dtype)
    nan = np.isnan(v).any(1)
    with np.errstate(invalid="ignore"):
        if asym:
            ub, lb = np.nanmax(v, 1), np.nanmin(v, 1)
        else:
            ub = np.nanmax(np.abs(v), 1)
            lb = -ub
    out = np.stack([ub, lb], 1)
    out[nan] = np.nan
    return out.astype(np.float32)
