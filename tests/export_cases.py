"""Shapes and inputs of the export kernels' launch-shape tests, shared by the CPU tier (tests/test_export_cases_cpu.py, which proves them
sensitive against deliberately wrong roundings, clamps, counts and packings) and the GPU tier (tests/test_gpu_export_shapes.py, which runs
fq_sym_export / fq_asym_export / fq_sym_row_scales on them).  numpy and torch-CPU only, no product code; the CPU oracle supplies the scales.

A row of `cols` elements is nvec = cols / EPV 16-byte vectors.  launch_export_reg (llm-qat_amd/csrc/fq_export.hip) picks a (threads per row,
vector slots per thread) instantiation of row_export_kernel from nvec with by_reg_shape (llm-qat_amd/csrc/fq_shapes.h), the ladder of the
forward kernels; a row that needs 5 (7) slots runs the 6 (8) slot instantiation, so every thread's last slot re-loads the row's last vector, and so does every slot at or beyond nvec in any other row.
Counted by the slots a row needs, the ladder has EIGHTEEN rungs (64 x {1, 2, 3}, 128 x {2, 3}, 256 x {2, 3}, 512 x {2, 3, 4, 5, 6, 7, 8} and
1024 x {5, 6, 7, 8}); all of them are listed here.

What fp16 cannot hold (and what the case builder gives it instead; the CPU tier asserts both):
  * outside autocast a row small enough for `+ 1e-6` to dominate its scale has 1 / (m + 1e-6) = Inf in fp16 (m + 1e-6 < 2^-16), and fp16's
    sub-normal grid (2^-24) is too coarse to place such a row's elements, so no saturating width has a mode-0 row other than -- under
    autocast and for Asym -- the row of zeros.  Its rows are mode 1 (while the full-scale bin qmax / S is below 65520: the product is rounded
    to fp16, so wider rows have the top bin Inf), mode 2, one `s = Inf` row (Sym; every bin +-Inf or
    NaN, all counted) and an all-zero row (Sym: 0 * Inf = NaN, all counted; Asym: 0 / 0 = NaN, all counted);
  * above 16 bits a finite Sym scale needs max|x| >= qmax / 65504, so the ordinary rows' magnitudes start there (2^15 at 31 bits).

Launch counts of the cross (one launch per combination and shape): bf16 22 x 54 = 1188; fp32 18 x 36 + 4 x 18 = 720 (no autocast on
fp32); fp16 22 x 36 + 6 x 18 = 900 -- the full COMBOS list at both 5-row widths of every rung, one fitting and one saturating pair per
arithmetic at the 1-, 3- and 4-row shapes.  2808 launches in all."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from group_cases import EPV, NAN, PINF, SIGN, MAXFIN, clip_predicate, differs, oracle_view, row_bounds, uint_of  # noqa: F401

# ---- the ladder: mirrors by_reg_shape (llm-qat_amd/csrc/fq_shapes.h; tests/test_shape_tables_cpu.py compares the two for every nvec) --
# lo < nvec <= hi runs row_export_kernel<TPR, slots>; vpt is the number of slots the row needs, slots the instantiation that runs (5 runs
# as 6, 7 as 8) ----------------------------------------------------------------------------------------------------------------------------
REG_MAX_VEC = 8192          # fq_shapes.h: wider rows take row_export_generic_kernel
Rung = namedtuple("Rung", "lo hi tpr vpt slots")
RUNGS = [Rung(0, 64, 64, 1, 1), Rung(64, 128, 64, 2, 2), Rung(128, 192, 64, 3, 3),
         Rung(192, 256, 128, 2, 2), Rung(256, 384, 128, 3, 3),
         Rung(384, 512, 256, 2, 2), Rung(512, 768, 256, 3, 3),
         Rung(768, 1024, 512, 2, 2), Rung(1024, 1536, 512, 3, 3), Rung(1536, 2048, 512, 4, 4), Rung(2048, 2560, 512, 5, 6),
         Rung(2560, 3072, 512, 6, 6), Rung(3072, 3584, 512, 7, 8), Rung(3584, 4096, 512, 8, 8),
         Rung(4096, 5120, 1024, 5, 6), Rung(5120, 6144, 1024, 6, 6), Rung(6144, 7168, 1024, 7, 8), Rung(7168, REG_MAX_VEC, 1024, 8, 8)]

Shape = namedtuple("Shape", "rung kind nvec rows cols")


def rung_of(nvec):
    return next(i for i, r in enumerate(RUNGS) if r.lo < nvec <= r.hi)


def widths(dtype):
    """per rung "dup" ((top - 1) * EPV: the last slot of the last thread is a clamped duplicate) and "tail" ((lower bound + 1) * EPV: the
    last slot-set holds one vector) at 5 rows; rows 1, 3 and 4 too on the three rungs that put four rows into one workgroup"""
    epv = EPV[dtype]
    out = []
    for i, r in enumerate(RUNGS):
        for rows in ((5, 1, 3, 4) if r.tpr == 64 else (5,)):
            out.append(Shape(i, "dup", r.hi - 1, rows, (r.hi - 1) * epv))
            out.append(Shape(i, "tail", r.lo + 1, rows, (r.lo + 1) * epv))
    return out


# ---- the combinations ------------------------------------------------------------------------------------------------------------------------
Combo = namedtuple("Combo", "kind bits container autocast")
CBITS = {"int4": 4, "int8": 8, "int16": 16}
_SYM = [(4, "int4"), (8, "int8"),                       # fitting; the bf16 +128 row
        (8, "int4"), (16, "int8"),                      # the specialised bodies, saturating
        (4, "int16"), (16, "int16"), (17, "int16"),     # the general body
        (23, "int16"), (24, "int8"),                    # the mode-1 / mode-2 threshold from both sides
        (31, "int4")]                                   # the widest accepted bit width
_SYM_AC = [(4, "int4"), (8, "int8"), (16, "int8"), (8, "int16")]        # the general body (autocast: bf16 / fp16 only)
_ASYM = [(4, "int4"), (8, "int8"), (16, "int16"),       # bins up to 65535
         (8, "int4"), (16, "int8"), (17, "int16"),      # saturating
         (22, "int16"), (23, "int16")]                  # the threshold from both sides
COMBOS = ([Combo("sym", b, c, False) for b, c in _SYM] + [Combo("sym", b, c, True) for b, c in _SYM_AC] +
          [Combo("asym", b, c, False) for b, c in _ASYM])
# one fitting and one saturating pair per arithmetic: what fp32 / fp16 run at the 1-, 3- and 4-row shapes
PAIRS = [Combo("sym", 8, "int8", False), Combo("sym", 16, "int8", False), Combo("sym", 8, "int8", True), Combo("sym", 16, "int8", True),
         Combo("asym", 8, "int8", False), Combo("asym", 16, "int8", False)]


def combos(dtype, kind=None, autocast=None):
    """fp32 has no autocast arithmetic: those combinations are absent, not skipped"""
    return [c for c in COMBOS if (dtype != "fp32" or not c.autocast) and kind in (None, c.kind) and autocast in (None, c.autocast)]


def body_of(c):
    """which export_row_body instantiation of row_export_kernel serves a combination"""
    if c.kind == "asym":
        return "asym"
    return c.container if (not c.autocast and c.container in ("int4", "int8")) else "general"


def cross(dtype, kind=None):
    """-> [(Combo, Shape)]: every combination at every shape for bf16; fp32 / fp16 the whole list at both 5-row widths of every rung and
    PAIRS at the 1-, 3- and 4-row shapes"""
    out = []
    for sh in widths(dtype):
        full = dtype == "bf16" or sh.rows == 5
        for c in (combos(dtype, kind) if full else [p for p in PAIRS if p in combos(dtype, kind)]):
            out.append((c, sh))
    return out


def crange(c):
    cb = CBITS[c.container]
    return (0, (1 << cb) - 1) if c.kind == "asym" else (-(1 << (cb - 1)), (1 << (cb - 1)) - 1)


def saturating(c):
    return c.bits > CBITS[c.container]


# ---- bit patterns <-> torch -------------------------------------------------------------------------------------------------------------------
TD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SIG = {"bf16": 8, "fp16": 11, "fp32": 24}      # significand bits


def to_f32(bits, dtype):
    """bit patterns -> float32 torch tensor (exact)"""
    a = np.ascontiguousarray(bits)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(np.int32 if dtype == "fp32" else np.int16)).view(TD[dtype]).float()


def from_f32(v, dtype):
    """float32 / float64 values -> bit patterns, one round-to-nearest-even"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float64))).to(torch.float32).to(TD[dtype]).contiguous()
    return t.view(torch.int32 if dtype == "fp32" else torch.int16).numpy().view(uint_of(dtype)).copy()


def neighbours(bits, dtype, w):
    """[n] patterns -> [n, 2 w + 1]: the dtype's grid around each value, in value order (finite patterns only)"""
    sign, top = int(SIGN[dtype]), int(MAXFIN[dtype])
    b = np.asarray(bits).astype(np.int64)
    mag = b & (sign - 1)
    key = np.where(b & sign, -mag, mag)[:, None] + np.arange(-w, w + 1)[None, :]
    key = np.clip(key, -top, top)
    return np.where(key < 0, (-key) | sign, key).astype(uint_of(dtype))


def pre_round(xbits, dtype, kind, nbits, autocast, scales):
    """what torch.round sees, [rows, n] float32: the reference's op order in fp32 with an explicit round to the tensor dtype after every op;
    Sym under autocast stays fp32 behind the reciprocal.  scales [rows, 2] are taken as given: Sym {s, t2}, Asym {alpha + 1e-8, beta}."""
    x = to_f32(xbits, dtype)
    sc = torch.from_numpy(np.array(scales, np.float32))
    rd = lambda t: t.to(TD[dtype]).float()  # noqa: E731
    if kind == "sym":
        p = x * sc[:, 0:1]
        return (p if autocast else rd(p)).numpy()
    S = torch.tensor(float(2 ** nbits - 1), dtype=torch.float32)
    return rd(rd(rd(x - sc[:, 1:2]) / sc[:, 0:1]) * S).numpy()


def restate(p, cmin, cmax):
    """pre_round -> (integers int64, bad bool): round half to even, NaN -> 0, saturate; bad = did not fit or was NaN"""
    q = np.rint(np.asarray(p, np.float64))
    nan = np.isnan(q)
    with np.errstate(invalid="ignore"):
        bad = nan | (q < cmin) | (q > cmax)
        ints = np.where(nan, 0, np.clip(q, cmin, cmax)).astype(np.int64)
    return ints, bad


def pack(ints, container):
    """integers [rows, cols] -> the packed bytes uint8 [rows, row_bytes] (int4: element 2k in the low nibble of byte k, two's complement)"""
    v = np.asarray(ints, np.int64)
    if container == "int8":
        return (v & 0xFF).astype(np.uint8)
    if container == "int16":
        out = np.empty((v.shape[0], v.shape[1] * 2), np.uint8)
        out[:, 0::2], out[:, 1::2] = v & 0xFF, (v >> 8) & 0xFF
        return out
    if v.shape[1] % 2:
        v = np.concatenate([v, np.zeros((v.shape[0], 1), np.int64)], 1)
    return ((v[:, 0::2] & 0xF) | ((v[:, 1::2] & 0xF) << 4)).astype(np.uint8)


def oracle_scales(bits, dtype, c, sem=None):
    from oracle import oracle as O
    rows, cols = bits.shape
    return O.export(c.kind, oracle_view(bits, dtype), rows, cols, c.bits, c.container, dtype, sem=sem, autocast=c.autocast)[1]


def row_modes(bits, dtype, c, scales):
    """the restated rule -> (top float64 [rows], mode int [rows]): the row's top bin is the bin of max|x| (Sym) / of the max (Asym);
    mode 0 iff top <= cmax, else 1 iff top < 2^22, else 2 (a NaN top is mode 2)"""
    ub = row_bounds(bits, dtype, c.kind == "asym")[:, 0:1]
    top = np.rint(pre_round(from_f32(ub, dtype), dtype, c.kind, c.bits, c.autocast, scales).astype(np.float64))[:, 0]
    cmax = crange(c)[1]
    with np.errstate(invalid="ignore"):
        mode = np.where(top <= cmax, 0, np.where(top < 4194304.0, 1, 2))
    return top, mode


# ---- the case builder -------------------------------------------------------------------------------------------------------------------------
Plant = namedtuple("Plant", "row col what arg")     # what: "bin" (arg = the unclamped bin), "frac_lo" / "frac_hi", "tie" (arg = the pre-round
#                                                     value), "pair" (arg = name; col is the even element of a byte), "negzero"
Built = namedtuple("Built", "bits plants rowkinds")
ROW_ORDER = ("pow2", "small", "special", "zero", "mid")     # rows 0 .. 4; fewer rows take a prefix.  The power-of-two row, whose ties every
#   case needs, comes first; a mode-0 row stands in front of the special row and of the last one (row 4, the first row of the second four-row
#   workgroup, is an ordinary row behind the row of zeros).  Below 5 rows a width of 22 bits or more has no mode-1 row: that is `mid`.


def hi_bits(c):
    """from here on an ordinary row's top bin is at or beyond 2^22 in some dtype: the `mid` row is made small enough for `+ 1e-6` / `+ 1e-8`
    to pull its top bin down to about 2^20, which is how a mode-1 row exists at these widths"""
    return c.bits >= 22


def pow2_exp(dtype, c, seed):
    if dtype == "fp16" and c.kind == "sym" and not c.autocast:
        qmax = 2.0 ** (c.bits - 1) - 1
        return max(5 + seed % 6, int(np.ceil(np.log2(qmax / 65504.0))))     # a finite scale needs max|x| >= qmax / 65504
    return 5 + seed % 6


def special_of(nvec, rows):
    """which special the `special` row of a case holds: the NaN at a rung's tail width and the +Inf at its dup width on even rungs, the
    other way round on odd rungs and at 4 rows, so that every rung and every row count that has the row meets both"""
    if not 0 < nvec <= REG_MAX_VEC:
        return "nan" if nvec % 2 == 0 else "pinf"
    i = rung_of(nvec)
    return "nan" if (i + (nvec == RUNGS[i].hi - 1) + (rows == 4)) % 2 == 0 else "pinf"


def row_kinds(dtype, c, rows):
    """names of the rows of a case (see export_inputs)"""
    small = "tiny"
    if dtype == "fp16":
        small = "sinf" if (c.kind == "sym" and not c.autocast) else "mid2"
    return [{"small": small}.get(n, n) for n in ROW_ORDER[:rows]]


@lru_cache(maxsize=None)
def _mid_for_top128():
    """a bf16 magnitude whose 8-bit Sym row has the top bin +128 (bf16 rounds 1 / m, then * 127, then m * s)"""
    c = Combo("sym", 8, "int8", False)
    cand = (np.arange(0x3F80, 0x4000, dtype=np.uint16))[:, None]          # [1, 2) on the bf16 grid
    top, _ = row_modes(cand, "bf16", c, oracle_scales(cand, "bf16", c))
    hit = np.flatnonzero(top == 128)
    assert hit.size
    return float(to_f32(cand[hit[len(hit) // 2]], "bf16")[0])


def _extremes(dtype, c, names, seed, special):
    """per row (mx, mn, special): the planted extremes as float64 (Sym: mn = -mx is the magnitude's mirror and only one of them is
    planted), special = None / "nan" / "pinf" / "zero" """
    cmax = crange(c)[1]
    qmax, S = 2.0 ** (c.bits - 1) - 1, 2.0 ** c.bits - 1
    k = pow2_exp(dtype, c, seed)
    mid = 1.37 * 2.0 ** (k - 1)
    if c == Combo("sym", 8, "int8", False) and dtype == "bf16":
        mid = _mid_for_top128() * 2.0 ** (k - 1)
    out = []
    for n in names:
        sp = None
        if n == "pow2":
            mx, mn = 2.0 ** k, -2.0 ** k
        elif n == "mid":
            mx, mn = mid, -0.83 * mid
            T = 2.0 ** 20
            if hi_bits(c) and dtype != "fp16":
                if c.kind == "sym":
                    mx = T * 1e-6 / (qmax - T)
                    mn = -mx
                else:
                    r = T * 1e-8 / (S - T)
                    mx, mn = 0.55 * r, -0.45 * r
        elif n == "mid2":
            mx, mn = 0.37 * mid, -0.21 * mid
        elif n == "tiny":
            if c.kind == "sym":
                mx = 0.8 * cmax * 1e-6 / qmax
                mn = -mx
            else:
                r = 0.8 * cmax * 1e-8 / S
                mx, mn = 0.55 * r, -0.45 * r
        elif n == "sinf":
            mx, mn = 2.0 ** -17, -2.0 ** -17
        elif n == "special":
            mx, mn = 0.61 * mid, -0.5 * mid
            sp = special
        else:
            mx = mn = 0.0
            sp = "zero"
        out.append((mx, mn, sp))
    return out


@lru_cache(maxsize=None)
def _all16():
    a = np.arange(65536, dtype=np.uint16)
    a.flags.writeable = False
    return a


@lru_cache(maxsize=None)
def _ties16(dtype, kind, bits, autocast, scale_bytes, lo, hi):
    """every 16-bit pattern between lo and hi under one row's scales -> ((pattern, pre-round value) or (None, None)) of a tie that rounds
    up, and of one that rounds down"""
    sc = np.frombuffer(scale_bytes, np.float32).reshape(1, 2)
    pa = pre_round(_all16()[None, :], dtype, kind, bits, autocast, sc)[0].astype(np.float64)
    out = []
    with np.errstate(invalid="ignore"):
        va = to_f32(_all16(), dtype).numpy().astype(np.float64)
        tie = (np.abs(pa - np.trunc(pa)) == 0.5) & (va >= lo) & (va <= hi)
        for ok in (tie & (np.rint(pa) > pa), tie & (np.rint(pa) < pa)):
            hit = np.flatnonzero(ok)
            out.append((int(hit[hit.size // 2]), float(pa[hit[hit.size // 2]])) if hit.size else (None, None))
    return tuple(out)


@lru_cache(maxsize=8)
def _filler(cols, rows):
    g = np.random.default_rng(cols * 31 + rows).standard_normal((rows, cols)).astype(np.float32)
    return np.clip(g, -3.0, 3.0) * np.float32(0.9 / 3.2)       # |g| <= 0.85


def _free(used, cols, start, step=1):
    p = start % cols
    for _ in range(cols):
        if p not in used:
            return p
        p = (p + step) % cols
    return None


@lru_cache(maxsize=48)
def _build(dtype, kind, bits, container, autocast, cols, rows):
    c = Combo(kind, bits, container, autocast)
    epv = EPV[dtype]
    u = uint_of(dtype)
    seed = cols // epv + rows + cols % epv
    names = row_kinds(dtype, c, rows)
    ext = _extremes(dtype, c, names, seed, special_of(cols // epv, rows))
    cmin, cmax = crange(c)
    asym = kind == "asym"

    # the extremes on the dtype's grid, and the oracle's scales of rows that hold just them
    eb = np.zeros((rows, 2), u)
    for r, (mx, mn, sp) in enumerate(ext):
        eb[r] = from_f32(np.array([mx, mn if (asym or cols == 1) else mx]), dtype)
        if not asym and (seed + r) % 2 and cols > 1:
            eb[r] |= u(SIGN[dtype])                # the Sym maximum is negative in every other row
        if cols == 1:
            eb[r, 1] = eb[r, 0]
    ev = to_f32(eb, dtype).numpy().astype(np.float64)
    scales = oracle_scales(eb, dtype, c)
    top, mode = row_modes(eb, dtype, c, scales)

    # filler between the extremes
    g = _filler(cols, rows).astype(np.float64)
    hi = np.maximum(ev[:, 0], ev[:, 1])[:, None]
    lo = np.minimum(ev[:, 0], ev[:, 1])[:, None]
    if not asym:
        hi = np.abs(ev[:, 0:1])
        lo = -hi
    x = from_f32((hi + lo) / 2 + g * (hi - lo) / 2, dtype)
    plants = []
    used = [set() for _ in range(rows)]

    def put(r, col, pattern, what, arg):
        if col is None:           # (a row of a few elements: no room left)
            return
        x[r, col] = pattern
        used[r].add(col)
        plants.append(Plant(r, col, what, arg))

    # extremes: the maximum in an early vector, the other extreme half a row away
    for r in range(rows):
        pmax = (seed * 5 + r * 3) % cols
        put(r, pmax, eb[r, 0], "max", None)
        if asym and cols > 1:
            put(r, _free(used[r], cols, pmax + cols // 2), eb[r, 1], "min", None)

    # search targets per row: edge bins, the fractions either side of cmax + 0.5, ties, the bin -1 (int4 nibble pairs)
    nvec = max(cols // epv, 1)
    finite = [n in ("mid", "mid2", "pow2", "tiny") for n in names]
    tg = []          # (what, arg, target value of the pre-round)
    for b in (cmax + 1, cmin - 1, cmax, cmin):
        tg.append(("bin", float(b), float(b)))
    tg.append(("frac_lo", None, cmax + 0.25))
    tg.append(("frac_hi", None, cmax + 0.75))
    if container == "int4" and not asym:
        tg.append(("bin", -1.0, -1.0))
    n_edge = len(tg)
    tie_small = [e + 0.5 for e in range(16)]
    per_row_t = []
    for r in range(rows):
        t = list(tg)
        tt = list(tie_small)
        if np.isfinite(top[r]):
            for f in (0.2, 0.3, 0.45, 0.6, 0.75, 0.9):
                e = 2.0 * np.floor(abs(top[r]) * f / 2.0)
                tt += [e + 0.5, e + 1.5]
        else:
            tt += [16.5 + i for i in range(12)]
        for v in tt:
            t.append(("tie", v, v))
            if not asym:
                t.append(("tie", -v, -v))
        if asym:
            t += [("tie", v + 16.0, v + 16.0) for v in tt]
        per_row_t.append(t)
    nt = len(per_row_t[0])
    W = 12
    tv = np.array([[t[2] for t in row] for row in per_row_t])                   # [rows, nt]
    s0, s1 = scales[:, 0:1].astype(np.float64), scales[:, 1:2].astype(np.float64)
    with np.errstate(all="ignore"):
        x0 = tv / s0 if not asym else tv / (2.0 ** bits - 1) * s0 + s1
    x0 = np.where(np.isfinite(x0), x0, 0.0)
    cand = neighbours(from_f32(x0.reshape(-1), dtype), dtype, W).reshape(rows, nt * (2 * W + 1))
    p = pre_round(cand, dtype, kind, bits, autocast, scales).astype(np.float64).reshape(rows, nt, 2 * W + 1)
    cv = to_f32(cand, dtype).numpy().astype(np.float64).reshape(rows, nt, 2 * W + 1)
    candb = cand.reshape(rows, nt, 2 * W + 1)
    order = np.argsort(np.abs(np.arange(-W, W + 1)), kind="stable")
    lastvec = (nvec - 1) * epv

    tie_seen = set()         # directions ("up" / "down") in which some planted tie of this case rounds
    for r in range(rows):
        if not finite[r] or cols < 2:
            continue
        inside = (cv[r] <= hi[r, 0]) & (cv[r] >= lo[r, 0])
        found = {}
        for ti, (what, arg, tval) in enumerate(per_row_t[r]):
            if what in ("bin", "frac_lo", "frac_hi") and ti < n_edge and mode[r] == 0 and not (what == "bin" and arg == -1.0):
                continue                                   # edges belong to mode-1 and mode-2 rows
            if what == "bin":
                ok = np.rint(p[r, ti]) == arg
            elif what == "frac_lo":
                ok = (p[r, ti] > cmax) & (p[r, ti] < cmax + 0.5)
            elif what == "frac_hi":
                ok = (p[r, ti] > cmax + 0.5) & (p[r, ti] < cmax + 1)
            else:
                ok = p[r, ti] == tval
            ok &= inside[ti]
            hit = [j for j in order if ok[j]]
            if hit:
                found[ti] = candb[r, ti, hit[0]]
        # where they go: the overflowing bin cmax + 1 into the row's LAST vector (a lane position that walks with cols), cmin - 1 (else cmax)
        # into vector 0, the rest spread over the row
        walk = (cols // epv * 3 + r) % epv
        spread = np.random.default_rng(seed * 977 + r).choice(cols, min(cols, 4 * nt + 16), replace=False)
        si = 0
        if mode[r] > 0 and 0 not in found:     # cmax + 1 is off this row's grid: the row's largest bin overflows too
            put(r, _free(used[r], cols, lastvec + walk), eb[r, 0] & ~u(0 if asym else SIGN[dtype]), "over", None)
        first_other = next((t for t in found if 0 < t < n_edge), None)
        for ti, pat in found.items():
            what, arg, _ = per_row_t[r][ti]
            if ti == 0:
                col = _free(used[r], cols, lastvec + walk)
                col = col if (col is None or col >= lastvec) else _free(used[r], cols, lastvec)
            elif ti == first_other:
                col = _free(used[r], cols, (walk + 1) % epv)
            else:
                col = _free(used[r], cols, int(spread[si % len(spread)]))
                si += 1
            if col is None:
                break
            put(r, col, pat, what, arg)
            if what == "tie":
                tie_seen.add("up" if np.rint(arg) > arg else "down")
        if names[r] == "pow2":          # +-2^(k-1) (Asym: 0): pre-round values +-qmax / 2 (S / 2), ties wherever the grid holds them
            half = from_f32(np.array([ev[r, 0] / 2, -ev[r, 0] / 2] if not asym else [0.0]), dtype)
            ph = pre_round(np.repeat(half[None, :], rows, 0), dtype, kind, bits, autocast, scales)[r]
            for pat, pv in zip(half, ph):
                col = _free(used[r], cols, int(spread[si % len(spread)]))
                si += 1
                if col is not None:
                    put(r, col, pat, "half", float(pv))
                    if abs(pv - np.trunc(pv)) == 0.5:
                        tie_seen.add("up" if np.rint(pv) > pv else "down")
        # a 16-bit grid is small enough to try every pattern: where the targets above gave no tie that rounds up (down), look for one
        if dtype != "fp32" and len(tie_seen) < 2:
            found16 = _ties16(dtype, kind, bits, autocast, scales[r].tobytes(), float(lo[r, 0]), float(hi[r, 0]))
            for name, (pat, pv) in zip(("up", "down"), found16):
                if name not in tie_seen and pat is not None:
                    col = _free(used[r], cols, int(spread[si % len(spread)]))
                    si += 1
                    put(r, col, u(pat), "tie", pv)
                    if col is not None:
                        tie_seen.add(name)
        # int4: nibble pairs at a byte position of a lane's packed word that walks with the row and the width
        if container == "int4" and cols >= 4 * epv:
            zero = u(0)
            if asym:
                pairs = [("max_min", eb[r, 0], eb[r, 1]), ("min_max", eb[r, 1], eb[r, 0])]
            else:
                big = eb[r, 0] & u(SIGN[dtype] - 1)
                neg = big | u(SIGN[dtype])
                pairs = [("neg_pos", neg, big), ("pos_neg", big, neg)]
                m1 = next((pat for ti, pat in found.items() if per_row_t[r][ti][:2] == ("bin", -1.0)), None)
                if m1 is not None:
                    pairs += [("m1_zero", m1, zero), ("zero_m1", zero, m1)]
            for pi, (name, a, b) in enumerate(pairs):
                bp = (seed + r + pi) % (epv // 2)
                v0 = (seed * 7 + r * 11 + pi * 5) % nvec
                col = None
                for dv in range(nvec):
                    q = ((v0 + dv) % nvec) * epv + 2 * bp
                    if q not in used[r] and q + 1 not in used[r]:
                        col = q
                        break
                if col is None:
                    continue
                x[r, col], x[r, col + 1] = a, b
                used[r].update((col, col + 1))
                plants.append(Plant(r, col, "pair", name))
        if r == 0:
            col = _free(used[r], cols, cols // 3)
            if col is not None:
                put(r, col, u(SIGN[dtype]), "negzero", None)

    for r, (_, _, sp) in enumerate(ext):
        if sp == "zero":
            x[r] = 0
            x[r, (seed + 2) % cols] = u(SIGN[dtype])
            plants.append(Plant(r, (seed + 2) % cols, "negzero", None))
        elif sp in ("nan", "pinf") and cols > 1:
            col = _free(used[r], cols, lastvec + (seed % epv) if seed % 3 else seed * 13)
            x[r, col] = u(NAN[dtype]) if sp == "nan" else u(PINF[dtype])
            plants.append(Plant(r, col, sp, None))
    x.flags.writeable = False
    return Built(x, tuple(plants), tuple(names))


def export_inputs(dtype, kind, bits, container, autocast, cols, rows):
    """bit patterns [rows, cols] of one case (memoised, read-only).  Rows, in order (fewer rows take a prefix):
      pow2     max|x| = 2^k, k >= 5 (Asym: max = -min = 2^k): s = qmax 2^-k wherever qmax fits the significand, with +-2^(k-1) (Asym: 0)
               planted, whose pre-round values +-qmax / 2 (S / 2) are ties
      tiny     magnitude 0.8 cmax 1e-6 / qmax (Asym: range 0.8 cmax 1e-8 / S): mode 0 at every width.  fp16: `sinf` (Sym outside
               autocast: max|x| = 2^-17, s = Inf) or `mid2` (another ordinary row)
      special  an ordinary row with one NaN or one +Inf (special_of: both at every rung, one per width): mode 2
      zero     zeros and one -0.0
      mid      an ordinary row, Gaussian filler between its planted extremes; from 22 bits on a row small enough for `+ 1e-6` (Asym
               `+ 1e-8`) to hold its top bin near 2^20, i.e. mode 1 where an ordinary row is mode 2 (not fp16: see the module text);
               bf16 Sym 8 -> int8: a magnitude whose top bin is +128; holds a -0.0
    Every mode-1 / mode-2 row with a finite scale holds elements whose unclamped bins are cmax + 1 (in the row's last vector), cmin - 1,
    cmax and cmin wherever they lie within the row's top bin and on the arithmetic's grid, pre-round values inside (cmax, cmax + 0.5) and
    (cmax + 0.5, cmax + 1) wherever that grid has them, and every exact tie the search finds (half-integers up to 15.5 and around six fractions of the row's top bin, either sign); int4 rows hold the nibble pairs of the
    packer's corner cases.  export_plants() lists what was planted where."""
    return _build(dtype, kind, bits, container, bool(autocast), cols, rows).bits


def export_plants(dtype, kind, bits, container, autocast, cols, rows):
    b = _build(dtype, kind, bits, container, bool(autocast), cols, rows)
    return b.plants, b.rowkinds


@lru_cache(maxsize=48)
def expected(dtype, kind, bits, container, autocast, cols, rows, sem=None):
    """memoised oracle.export of a case -> (bytes uint8 [rows, row_bytes], scales float32 [rows, 2], overflow int32 [rows]), read-only"""
    from oracle import oracle as O
    x = export_inputs(dtype, kind, bits, container, autocast, cols, rows)
    out = O.export(kind, oracle_view(x, dtype), rows, cols, bits, container, dtype, sem=sem, autocast=bool(autocast))
    for a in out:
        a.flags.writeable = False
    return out


def unclamped(dtype, kind, bits, autocast, x):
    """the oracle's unclamped bins int32 [rows, cols] (NaN -> INT32_MIN, +-Inf -> +-INT32_MAX)"""
    from oracle import oracle as O
    rows, cols = x.shape
    if kind == "asym":
        return O.asym_fwd(oracle_view(x, dtype), rows, cols, bits, dtype, want_idx=True)[1].reshape(rows, cols)
    if autocast:
        return O.sym_fwd_autocast(oracle_view(x, dtype), rows, cols, bits, dtype)[1].reshape(rows, cols)
    return O.sym_fwd(oracle_view(x, dtype), rows, cols, bits, dtype, want_idx=True)[1].reshape(rows, cols)


def scales_equal(got, want, asym):
    """scales as bits; the one relaxation: Asym beta may differ in the sign of zero (-0.0 and +0.0 are equal minima)"""
    g, w = np.array(got, np.float32), np.array(want, np.float32)
    if asym:
        g[:, 1][g[:, 1] == 0] = 0.0
        w[:, 1][w[:, 1] == 0] = 0.0
    return not differs(g.view(np.uint32), w.view(np.uint32), "fp32").any()
