"""The launch ladder of the two register-ladder row kernels, mirrored once, and the case lists that walk it: the attention softmax
(fq_attn_softmax.h / .hip) and the RMSNorm (fq_rms_norm.h / .hip, section 25).  Torch only, no product code.

The host side chooses, from the column count, the storage dtype and the alignment of every pointer and stride: a wave or a workgroup per
row (by_row_shape), the 16-byte or the element path, on the 16-byte path one of three kernels built for a quarter, a half and all of
*_VIF vectors per lane, and rows wider than a sweep loop over it.  cell() is that choice in Python.  Its constants are read out of the
headers by regular expressions (header_constants), never typed in here, so a retuned macro moves the case lists with it, and
tests/test_row_ladder_cases_cpu.py pins what the lists hold at today's constants.

A cell is (path, TPR, slots per lane, sweeps, groups in the last sweep); its class (cell_class) caps the sweeps at three and leaves the
group count out: every kernel instance, at one, two and three or more sweeps.  The case lists hold the first and the last column count
of every class, so both sides of every boundary.

Inputs.  A random row does not make a miscounted slot visible above a cap, so row 0 of every case is seeded: its largest value lies in
column 0 (in group 0 whatever the path: what a slot past the row re-reads in a single sweep), its second largest in the last column
(what a dropped last group loses), its third in the first column of the last sweep under every path the column count can take (what a
slot past the row re-reads in a later sweep).  For the softmax each is within 1.0 of the maximum after scaling, so each carries an O(1)
share of the sum, and g is largest in magnitude at the same columns.  For the norm the three hold the row's largest magnitudes.  Where
a row is wider than a sweep, row 1 of a softmax case holds its maximum in the first column of the last sweep, more than 89 above the
rest after scaling: a maximum taken without the last sweep is wrong in the stats and overflows fp32's exponential.  The other rows are
randn, bf16-representable as the reference modules' _case makes them.
"""
import functools
import math
import os
import re
from collections import namedtuple

import torch

import attn_softmax_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llm-qat_amd", "csrc")
WAVE = 64                                                            # lanes of a wave: the TPR of a row that is not wide
BF, H, F = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, H, F]
ESIZE = {BF: 2, H: 2, F: 4}

_WHERE = {
    "ROW_WIDE": ("fq_rows.h", r"constexpr\s+int64_t\s+ROW_WIDE\s*=\s*(\d+)\s*;"),
    "ROW_TPB": ("fq_rows.h", r"constexpr\s+int\s+ROW_TPB\s*=\s*(\d+)\s*;"),
    "ATTN_VIF": ("fq_attn_softmax.h", r"#define\s+ATTN_VIF\s+(\d+)\b"),
    "ATTN_EG": ("fq_attn_softmax.h", r"constexpr\s+int\s+ATTN_EG\s*=\s*(\d+)\s*;"),
    "RMS_VIF": ("fq_rms_norm.h", r"#define\s+RMS_VIF\s+(\d+)\b"),
    "RMS_EG": ("fq_rms_norm.h", r"constexpr\s+int\s+RMS_EG\s*=\s*(\d+)\s*;"),
}


def header_constants():
    """name -> int, each defined exactly once in its header (else a ValueError: the mirror has lost its source)"""
    out = {}
    for name, (fname, pattern) in _WHERE.items():
        found = re.findall(pattern, open(os.path.join(CSRC, fname)).read())
        if len(found) != 1:
            raise ValueError(f"{name}: {len(found)} definitions in {fname}, expected one")
        out[name] = int(found[0])
    return out


K = header_constants()
FAMILY = {"attn": ("ATTN_VIF", "ATTN_EG"), "rms": ("RMS_VIF", "RMS_EG")}

Cell = namedtuple("Cell", "path tpr slots sweeps last_groups")


def geometry(cols, dtype, aligned, family="attn"):
    """-> (path, TPR, EPV, groups of a lane per sweep): by_row_shape, row_vec / attn_vec's condition on cols, by_attn_kernel / by_rms_kernel.
    aligned: every base pointer and every stride is a multiple of 16 bytes (and, for the norm, x and w share the dtype)"""
    vif, eg = (K[n] for n in FAMILY[family])
    esize = ESIZE[dtype]
    tpr = K["ROW_TPB"] if cols >= K["ROW_WIDE"] else WAVE
    if not (aligned and cols * esize % 16 == 0):
        return "elt", tpr, 1, eg
    most = vif * esize // 2
    need = (cols * esize // 16 + tpr - 1) // tpr                     # vectors of a lane
    for step in (2, 1):
        ng = max(most >> step, 1)
        if need <= ng:
            return "vec", tpr, 16 // esize, ng
    return "vec", tpr, 16 // esize, most


def cell(cols, dtype, aligned, family="attn"):
    path, tpr, epv, ng = geometry(cols, dtype, aligned, family)
    sweep = ng * epv * tpr
    sweeps = -(-cols // sweep)
    return Cell(path, tpr, ng * epv, sweeps, -(-(cols - (sweeps - 1) * sweep) // epv))


def last_sweep(cols, dtype, aligned, family="attn"):
    """-> (first column of the last sweep, columns of a group, does the last sweep hold a slot past the row)"""
    path, tpr, epv, ng = geometry(cols, dtype, aligned, family)
    sweep = ng * epv * tpr
    c0 = (-(-cols // sweep) - 1) * sweep
    return c0, epv, cols - c0 < sweep


def cell_class(c):
    return (c.path, c.tpr, c.slots, min(c.sweeps, 3))


def _scan_limit(family):
    """three sweeps of the widest kernel and a group more: every class there is starts below it"""
    vif, eg = (K[n] for n in FAMILY[family])
    return 3 * max(vif * 8, eg) * K["ROW_TPB"] + 16


@functools.lru_cache(maxsize=None)
def classes(dtype, family="attn"):
    """class -> [first, last] column count, over every column count and both alignments: all the mirror can produce"""
    out = {}
    for aligned in (True, False):
        for cols in range(1, _scan_limit(family) + 1):
            k = cell_class(cell(cols, dtype, aligned, family))
            if k[0] == ("vec" if aligned else "elt"):
                out.setdefault(k, [cols, cols])[1] = cols
    return out


def _edges(dtype, family, path):
    """the first and the last column count of every class of `path`; of the class that has no end, three sweeps or more, the first"""
    cols = set()
    for k, (first, last) in classes(dtype, family).items():
        if k[0] == path:
            cols.add(first)
            if last < _scan_limit(family):
                cols.add(last)
    return cols


def attn_cols(dtype):
    """-> (aligned, element): the sorted column counts of the attention softmax's cases for scores of `dtype`.  aligned: the 16-byte path,
    every class's first and last count; fp32 also runs the 16-bit counts, so that one count is seen under every dtype.  element: reached
    by an odd count or by a base offset of one element; every class's first and last count, and where a last count is whole 16-bit vectors
    the count below it, which takes the path by itself"""
    vec = _edges(dtype, "attn", "vec")
    if dtype is F:
        vec |= _edges(BF, "attn", "vec")
    elt = _edges(dtype, "attn", "elt")
    elt |= {c - 1 for c in elt if c % 8 == 0}
    return sorted(vec), sorted(elt)


def all_attn_cols():
    """every column count of the GPU tier -> {cols: needs the run at a base offset of one element}"""
    out = {}
    for dtype in DTYPES:
        vec, elt = attn_cols(dtype)
        for c in vec:
            out.setdefault(c, False)
        for c in elt:
            out[c] = True
    return dict(sorted(out.items()))


def rows_of(cols):
    """one full workgroup of four rows and a partial one on the wave path; three workgroups else"""
    return 3 if cols >= K["ROW_WIDE"] else 5


def rms_new_cols(dtype):
    """what the norm's GPU tier adds to its SHAPES: the wave path's classes on the 16-byte path, first and last count each (SHAPES holds
    8, 64 and 256 columns of them, the quarter rung only), the workgroup's full rung filled exactly, and the first count of a third sweep"""
    out = set()
    todo = [dtype] + ([BF] if dtype is F else [])
    for dt in todo:
        for k, (first, last) in classes(dt, "rms").items():
            if k[0] == "vec" and k[1] == WAVE:
                out |= {first, last}
            if k == ("vec", K["ROW_TPB"], 8 * K["RMS_VIF"], 1):      # all of RMS_VIF vectors, one sweep
                out.add(last)
            if k == ("vec", K["ROW_TPB"], 8 * K["RMS_VIF"], 3):      # a third sweep, one group in it (SHAPES ends at 11008 columns)
                out.add(first)
    return sorted(out)


def rms_cells_reached(dtype, shapes):
    """the classes that `shapes` ([(rows, cols)]) reach on the 16-byte path and, by the offset and the odd counts, on the element path"""
    return {cell_class(cell(c, dtype, a, "rms")) for _, c in shapes for a in (True, False)}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def planted_columns(cols, family="attn"):
    """-> (first, last, thirds): column 0, the last column, and the first column of the last sweep under every path and dtype the count
    can take (where that is neither of the two)"""
    thirds = set()
    for dtype in DTYPES:
        for aligned in (True, False):
            thirds.add(last_sweep(cols, dtype, aligned, family)[0])
    return 0, cols - 1, sorted(thirds - {0, cols - 1})


def far_column(cols):
    """the first column of the last sweep where a row is wider than a sweep under some path (the latest such), else None"""
    c0 = max(last_sweep(cols, dtype, aligned)[0] for dtype in DTYPES for aligned in (True, False))
    return c0 if c0 > 0 else None


TOP = (192.0, 186.0, 184.0)                                          # scores: z = 16.97, 16.44, 16.26 at HEAD_DIM 128, the rest N(0, 0.71)
G_TOP = (8.0, -6.0, 5.0)
FAR = 1280.0                                                         # z = 113: e^(z - max of the rest) is beyond fp32


def attn_inputs(cols, rows=None, masked=True, seed=None):
    """-> (scores fp32 [1, 1, rows, cols], keep bool [1, 1, rows, cols] or None, g fp32) on the CPU, bf16-representable.  keep: the
    unmasked columns, 70 % of them, column 0 of every row and the planted columns"""
    rows = rows_of(cols) if rows is None else rows
    gen = torch.Generator().manual_seed(29000 + cols if seed is None else seed)
    x = (torch.randn((1, 1, rows, cols), generator=gen) * 8).bfloat16().float()
    g = torch.randn((1, 1, rows, cols), generator=gen).bfloat16().float()
    keep = torch.rand((1, 1, rows, cols), generator=gen) < 0.7
    keep[..., 0] = True
    first, last, thirds = planted_columns(cols)
    for col, v, gv in [(c, TOP[2], G_TOP[2]) for c in thirds] + [(last, TOP[1], G_TOP[1]), (first, TOP[0], G_TOP[0])]:
        x[0, 0, 0, col], g[0, 0, 0, col], keep[0, 0, 0, col] = v, gv, True
    if far_column(cols) is not None and rows > 1:
        x[0, 0, 1, far_column(cols)], keep[0, 0, 1, far_column(cols)] = FAR, True
    return x, (keep if masked else None), g


def attn_mask(keep, dtype, device="cpu"):
    return None if keep is None else torch.where(keep, 0.0, torch.finfo(dtype).min).to(dtype).to(device)


RMS_SIGMA = 1.5


def rms_inputs(cols, rows=None, seed=None):
    """-> x [rows, cols], w [cols], g fp32 on the CPU, bf16-representable; row 0 holds 8 sigma at the planted columns"""
    rows = rows_of(cols) if rows is None else rows
    gen = torch.Generator().manual_seed(25000 + cols if seed is None else seed)
    x = (torch.randn((rows, cols), generator=gen) * RMS_SIGMA).bfloat16().float()
    w = (1 + 0.1 * torch.randn(cols, generator=gen)).bfloat16().float()
    g = torch.randn((rows, cols), generator=gen).bfloat16().float()
    first, last, thirds = planted_columns(cols, "rms")
    for col, sign in [(c, 1.0) for c in thirds] + [(last, -1.0), (first, 1.0)]:
        x[0, col] = sign * 8 * RMS_SIGMA
    return x, w, g


# ---- the measures on float64 results ------------------------------------------------------------------------------------------------------
def c_y64(y, ref, dtype):
    """attn_softmax_reference.c_y of a float64 y held to `dtype`'s one output rounding"""
    return float(A._ratio(A._excess(y, ref["p"], dtype, 1), ref["p"]).max() / A.UNIT)


def c_dx64(dx, ref, dtype):
    p, g = ref["p"], ref["g"]
    den = ref["inv"] * p * (g.abs() + (g * p).abs().sum(-1, keepdim=True))
    return float(A._ratio(A._excess(dx, ref["dx"], dtype, 2), den).max() / A.UNIT)


def exceeds(measure, cap):
    """a NaN measure exceeds every cap: the tests assert measure <= cap"""
    return not measure <= cap


def softmax_with(ref, add_cols=None, drop_cols=None, max_below=None):
    """the float64 softmax of ref's row 0 ... rows, with a fault in the reduction -> (p, dx by the recipe from that p, the maximum used).
    add_cols: these columns' terms counted once more in the sum; drop_cols: left out of it; max_below: the maximum taken over the
    columns below this one alone, and the exponentials in fp32, where the kernels take them"""
    a = ref["a"]
    z = a if ref["min"] is None else a.clamp_min(ref["min"])
    m = (z if max_below is None else z[..., :max_below]).amax(-1, keepdim=True)
    e = torch.exp(z - m) if max_below is None else torch.exp((z - m).float()).double()
    s = e.sum(-1, keepdim=True)
    if add_cols is not None:
        s = s + e[..., add_cols[0]:add_cols[1]].sum(-1, keepdim=True)
    if drop_cols is not None:
        s = s - e[..., drop_cols[0]:drop_cols[1]].sum(-1, keepdim=True)
    p = e / s
    return p, A.recipe64(dict(ref, p=p)), m


def row_stats64(scores, mask, head_dim=A.HEAD_DIM):
    """-> (max, sum of exp(z - max)) per row in float64, of z_of's exact values"""
    z = A.z_of(scores, mask, head_dim)[1].double()
    m = z.amax(-1)
    return m.reshape(-1), torch.exp(z - m.unsqueeze(-1)).sum(-1).reshape(-1)


assert math.sqrt(A.HEAD_DIM) * 89 < FAR - 6 * 8                      # FAR stands 89 above six sigma of the rest after scaling: fp32 exp overflows at 88.7
