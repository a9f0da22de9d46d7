"""Inputs, expected values and memory layouts of the row kernels' launch-shape tests, shared by the contiguous walk
(tests/test_gpu_row_launch_shapes.py, tests/test_gpu_stage_kernels.py), the pitched and multi-tensor walks (tests/test_gpu_row_views.py,
tests/test_gpu_row_multi.py), the non-temporal-load worker (tests/row_ntl_worker.py) and the CPU tier that proves the layouts sensitive
(tests/test_row_view_cases_cpu.py).  numpy only, no product code: expected values come from the CPU oracle (oracle/oracle.py), the clip
predicate on x and group_cases.row_bounds / clip_predicate / grad_bits.

A width is cols = (nvec - 1) * EPV for a rung whose rows hold up to nvec 16-byte vectors, so the last lane slot of the row is the clamped
duplicate of the last vector; 5 rows (6 where a 3-D view needs a product), so the kernels that put four rows into a workgroup run a partly
empty last one.

A View is (offset, n_inner, stride_outer, stride_inner) in ELEMENTS with fq_rows_view's meaning: row r of the [rows, cols] view starts
offset + (r / n_inner) * stride_outer + (r % n_inner) * stride_inner elements behind the start of its buffer; n_inner = 0: contiguous."""
from collections import namedtuple

import numpy as np

import group_cases as C
from mx_reference import encode

ROWS = 5
LO, HI = -2.0, 2.0
BITS = 4
# threads per row -> the nvec at the top of each of its rungs (fq_shapes.h by_reg_shape)
RUNGS = {64: (64, 128, 192), 128: (256, 384), 256: (512, 768), 512: (1024, 1536, 2048, 2560, 3072, 3584, 4096), 1024: (5120, 6144, 7168, 8192)}
NVECS = [n for tpr in RUNGS for n in RUNGS[tpr]]
# fp32-result forward (launch_wide): nh = cols / 4 half-vectors per row, hpt = ceil(nh / TPR) of them per thread; TPR 64 up to nh = 512,
# 256 up to 2048, then 1024.  nh = TPR * hpt - 2: the last slot is a clamped duplicate, and cols stays a multiple of 8 (the bitmap's unit).
WIDE_NH = [64 * h - 2 for h in range(1, 9)] + [256 * h - 2 for h in range(3, 9)] + [1024 * h - 2 for h in range(3, 9)]
# fp32-gradient backward (launch_ste_mask_wide): one chunk up to nh = 2048, hpt = ceil(nh / 256) = 1 .. 8 (the TPR 256 widths above are
# hpt 3 .. 8 of it; these are 1 and 2)
WIDE_BWD_NH = [256 * h - 2 for h in range(1, 9)]
# rows of 256 v - 1 vectors: v vectors per thread (launch_ste_rows), the last lane slot a clamped duplicate; 2049 vectors: two chunks of
# 1025 and 1024 vectors at 5 vectors per thread, the second one short
ROW_NVECS = [256 * v - 1 for v in range(1, 9)] + [2049]
# the mask backward (launch_ste_mask): one top-of-rung nvec per vectors-per-thread count 1 .. 8 (backward_vpt(n - 1)); 2560, 3584 and
# 4096 run two chunks per row
MASK_BWD_NVECS = [64, 384, 768, 1024, 2560, 1536, 3584, 4096]


# ---- inputs and expected values: numpy and the oracle only, computed once per process -------------------------------------------------------

_memo = {}


def memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _memo:
            v = fn(*key)
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
            _memo[k] = v
        return _memo[k]
    return wrapped


@memo
def row_bits(dt, cols, rows=ROWS):
    """bit patterns [rows, cols]: even rows cross the clip +-2, odd rows stay well inside it; row 0 holds +-2 and the patterns one ulp on
    either side of them and a -0.0, some of them in the row's last vector; row 2 (if there is one) a NaN there"""
    u = C.uint_of(dt)
    rng = np.random.default_rng(cols * 7 + rows)
    v = rng.standard_normal((rows, cols)) * np.where(np.arange(rows) % 2 == 0, 1.5, 0.25)[:, None]
    b = encode(v.astype(np.float32).astype(np.float64), dt).astype(u)
    two, sign = u(C.TWO[dt]), u(C.SIGN[dt])
    edge = [two, two | sign, two + u(1), two - u(1), (two + u(1)) | sign, (two - u(1)) | sign, sign]
    where = [3, cols // 2, cols // 3, cols - 1, cols - 2, 0, cols - 3]
    for p, val in zip(where, edge):
        b[0, p] = val
    if rows > 2:
        b[2, cols - 4] = C.NAN[dt]
    return b


@memo
def forward_reference(dt, kind, cols, rows=ROWS):
    from oracle import oracle as O
    fn = O.sym_fwd if kind == "sym" else O.asym_fwd
    return fn(C.oracle_view(row_bits(dt, cols, rows), dt), rows, cols, BITS, dt, sem=0, want_idx=False)[0].view(C.uint_of(dt)).reshape(rows, cols)


@memo
def autocast_reference(dt, wide, cols, rows=ROWS):
    """the oracle the autocast tests use: bit patterns of the tensor dtype, or (wide) of the fp32 result"""
    from oracle import oracle as O
    y = O.sym_fwd_autocast(row_bits(dt, cols, rows), rows, cols, BITS, dt, wide=wide)[0]
    return y.view(np.uint32 if wide else np.uint16).reshape(rows, cols)


@memo
def side_reference(dt, asym, cols, rows=ROWS):
    """-> (bounds float32 [rows, 2] as bits, clippable rows, predicate bool [rows, cols])"""
    b = row_bits(dt, cols, rows)
    bounds = C.row_bounds(b, dt, asym)
    clippable = ~((bounds[:, 0] < HI) & (bounds[:, 1] > LO))
    assert clippable.any() and (~clippable).any()
    return bounds.view(np.uint32), clippable, C.clip_predicate(b, dt, LO, HI)


@memo
def grad_and_masked(dt, cols, rows=ROWS):
    """a gradient with NaN, +-Inf and -0.0 at zeroed and at kept positions, and that gradient with +0.0 where the predicate holds"""
    pred = C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI)
    g = C.grad_bits(pred, dt, cols + rows)
    want = g.copy()
    want[pred] = 0
    return g, want


@memo
def wide_grad_and_cast(dt, cols, rows=ROWS):
    """the fp32 gradient of a fp32-result forward, and its rounding to the input's dtype (torch's CPU cast)"""
    import torch
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    g = C.grad_bits(C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI), "fp32", cols + rows)
    return g, torch.from_numpy(g.view(np.float32).copy()).to(tdt).view(torch.int16).numpy().view(np.uint16).copy()


@memo
def wide_grad_and_masked(dt, cols, rows=ROWS):
    """... and that rounding with +0.0 where the predicate holds"""
    g, cast = wide_grad_and_cast(dt, cols, rows)
    want = cast.copy()
    want[C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI)] = 0
    return g, want


def backward_vpt(nvec_row):
    """launch_ste_mask's vectors per thread for a row of nvec_row vectors"""
    chunks = (nvec_row + 2047) // 2048
    cv = ((nvec_row + chunks - 1) // chunks + 63) // 64 * 64
    return (cv + 255) // 256


def rows_vpt(nvec_row):
    """launch_ste_rows's vectors per thread"""
    chunks = (nvec_row + 2047) // 2048
    return ((nvec_row + chunks - 1) // chunks + 255) // 256


def wide_shape(nh):
    """launch_wide's (threads per row, half-vectors per thread) for a row of nh half-vectors (7 per thread run the 8 kernel)"""
    tpr = 64 if nh <= 512 else 256 if nh <= 2048 else 1024
    return tpr, -(-nh // tpr)


# ---- expected values at any bit width, for the multi-tensor and the debug forwards ------------------------------------------------------

@memo
def sym_reference(dt, mode, cols, rows, bits):
    """SymQuantizer on row_bits(dt, cols, rows) at `bits`: mode 0 the plain arithmetic (cpu_eager), 1 / 2 the autocast arithmetic rounded
    to the tensor dtype / as the fp32 result -> bit patterns [rows, cols]"""
    from oracle import oracle as O
    b = row_bits(dt, cols, rows)
    if mode == 0:
        return O.sym_fwd(C.oracle_view(b, dt), rows, cols, bits, dt, sem=0, want_idx=False)[0].view(C.uint_of(dt)).reshape(rows, cols)
    y = O.sym_fwd_autocast(b, rows, cols, bits, dt, wide=mode == 2)[0]
    return y.view(np.uint32 if mode == 2 else np.uint16).reshape(rows, cols)


@memo
def debug_reference(dt, kind, cols, rows=ROWS):
    """-> (y bits [rows, cols], idx int32 [rows, cols], scales float32 bits: Sym [rows], Asym [rows, 2] = {alpha, beta})"""
    from oracle import oracle as O
    xv = C.oracle_view(row_bits(dt, cols, rows), dt)
    if kind == "sym":
        y, idx, s = O.sym_fwd(xv, rows, cols, BITS, dt, sem=0)
        sc = s
    else:
        y, idx, al, be = O.asym_fwd(xv, rows, cols, BITS, dt, sem=0)
        sc = np.stack([al, be], 1)
    return y.view(C.uint_of(dt)).reshape(rows, cols), idx.reshape(rows, cols), np.ascontiguousarray(sc).view(np.uint32)


@memo
def side_expected(dt, asym, cols, rows):
    """side_reference for any row count (a one-row tensor has no unclippable row): bounds bits, clippable rows, predicate"""
    b = row_bits(dt, cols, rows)
    bounds = C.row_bounds(b, dt, asym)
    return bounds.view(np.uint32), ~((bounds[:, 0] < HI) & (bounds[:, 1] > LO)), C.clip_predicate(b, dt, LO, HI)


def mask_row_bytes(cols):
    return (cols + 63) // 64 * 8


def side_bytes(dt, asym, cols, rows, junk=0xFF):
    """the side buffer a training forward leaves (float32 bounds [rows][2], then the row bitmap), built from the predicate: uint8.  The
    bitmap rows of unclippable rows, which no forward writes and no backward may read, hold `junk`."""
    bounds, clippable, pred = side_expected(dt, asym, cols, rows)
    m = np.full((rows, mask_row_bytes(cols)), junk, np.uint8)
    packed = np.packbits(pred, axis=1, bitorder="little")
    for r in np.flatnonzero(clippable):
        m[r] = 0
        m[r, : packed.shape[1]] = packed[r]
    return np.concatenate([np.ascontiguousarray(bounds).view(np.uint8).reshape(-1), m.reshape(-1)])


# ---- memory layouts --------------------------------------------------------------------------------------------------------------------

View = namedtuple("View", "offset n_inner stride_outer stride_inner")
CONTIG = View(0, 0, 0, 0)
GUARD = 16                      # canary elements behind the last addressed one of every destination buffer
CANARY = {"bf16": 0x5A5B, "fp16": 0x5A5B, "fp32": 0x5A5B5C5D}
LAYOUTS_2D = ("contig", "slice", "every_other", "expanded", "half")
LAYOUTS_3D = ("transposed", "padded")


def rows_of(layout):
    return 6 if layout in LAYOUTS_3D else ROWS


def layout(name, cols, epv, rows=None):
    """the View of a named layout for rows of `cols` elements whose 16-byte vector holds `epv` of them.  Every row start is a multiple of
    epv (16-byte aligned) except in "half", whose offset and strides are 4 mod 8 elements (16-bit tensors: 8-byte aligned)."""
    rows = rows_of(name) if rows is None else rows
    if name == "contig":
        return CONTIG
    if name == "slice":                 # [:, epv : epv + cols] of a [rows, cols + 3 epv] tensor
        return View(epv, rows, 0, cols + 3 * epv)
    if name == "every_other":           # [::2] of a [2 rows, cols] tensor
        return View(0, rows, 0, 2 * cols)
    if name == "expanded":              # expand() of one row: sources only
        return View(epv, rows, 0, 0)
    if name == "half":
        assert epv == 8 and cols % 8 == 0
        return View(4, rows, 0, cols + 12)
    w = cols + 2 * epv
    if name == "transposed":            # [2, 3, cols] = transpose(0, 1) of a [3, 2, cols + 2 epv] buffer: stride_outer < stride_inner
        assert rows == 6
        return View(0, 3, w, 2 * w)
    if name == "padded":                # [2, 3, cols] inside a larger 3-D buffer: stride_outer > stride_inner > cols
        assert rows == 6
        return View(2 * epv, 3, 3 * w + epv, w)
    raise KeyError(name)


def row_starts(view, rows, cols):
    """element index of every row's first element: the statement of fq_rows_view the kernels are held to"""
    r = np.arange(rows, dtype=np.int64)
    if view.n_inner == 0:
        return view.offset + r * cols
    return view.offset + (r // view.n_inner) * view.stride_outer + (r % view.n_inner) * view.stride_inner


def buffer_elems(view, rows, cols):
    """the smallest buffer that holds every addressed element"""
    return int(row_starts(view, rows, cols).max()) + cols


def addressed(view, rows, cols, n):
    """bool [n]: the elements some row addresses"""
    m = np.zeros(n, bool)
    for s in row_starts(view, rows, cols):
        m[s: s + cols] = True
    return m


def gather(buffer, view, rows, cols):
    return np.stack([buffer[s: s + cols] for s in row_starts(view, rows, cols)])


def scatter_expected(want, view, dt, n=None):
    """the destination buffer a correct launch leaves: `want`'s rows where the view puts them, the canary everywhere else (GUARD elements
    behind the last row included)"""
    rows, cols = want.shape
    n = buffer_elems(view, rows, cols) + GUARD if n is None else n
    buf = np.full(n, CANARY[dt], C.uint_of(dt))
    for r, s in enumerate(row_starts(view, rows, cols)):
        buf[s: s + cols] = want[r]
    return buf


def hostile(dt):
    """a finite magnitude above every row's maximum (12288) and a NaN"""
    u = C.uint_of(dt)
    return u(encode(np.array([12288.0]), dt)[0]), u(C.NAN[dt])


def source_buffer(data, view, dt):
    """-> (buffer, rows as the view addresses them).  Elements no row addresses hold a magnitude above every row's maximum, the first
    element of every such gap (and of the GUARD elements at the end) a NaN: read by mistake they change the row's statistics, its values or
    its gradient.  Rows that share their memory (stride 0) all hold data's first row."""
    rows, cols = data.shape
    n = buffer_elems(view, rows, cols) + GUARD
    big, nan = hostile(dt)
    buf = np.full(n, big, C.uint_of(dt))
    for r, s in reversed(list(enumerate(row_starts(view, rows, cols)))):
        buf[s: s + cols] = data[r]
    used = addressed(view, rows, cols, n)
    gap_start = ~used & np.concatenate([[True], used[:-1]])
    buf[gap_start] = nan
    return buf, gather(buf, view, rows, cols)


def as_addressed(want, view):
    """expected rows for a source in `view`: rows that share their memory all give the first row's result"""
    if view.n_inner and view.stride_inner == 0 and view.stride_outer == 0:
        return np.repeat(want[:1], want.shape[0], axis=0)
    return want


# (name, source layout, destination layout): a pitched source with a contiguous destination, a contiguous source with a pitched
# destination, both pitched with different views, both 3-D orders, and an expanded source
PAIRINGS = [("src_slice", "slice", "contig"), ("dst_slice", "contig", "slice"), ("src_other_dst_slice", "every_other", "slice"),
            ("src_transposed_dst_padded", "transposed", "padded"), ("src_padded_dst_transposed", "padded", "transposed"),
            ("src_expanded_dst_other", "expanded", "every_other")]
# where the launch layer accepts 8-byte aligned rows: x of the fp32-result forward, gx of the fp32-gradient backward
HALF_SRC = ("src_half", "half", "contig")
HALF_DST = ("dst_half", "every_other", "half")     # (a fp32 "slice" has the same numbers as "half": the exchanged views would go unseen)
# an in-place backward has one view for g and gx
INPLACE_LAYOUTS = ("slice", "every_other", "transposed", "padded")
# fq_ste_bwd_v: (g, x, gx)
TRIPLES = [("g_slice_x_other", "slice", "every_other", "contig"), ("gx_slice", "contig", "contig", "slice"),
           ("g_transposed_x_slice_gx_padded", "transposed", "slice", "padded"), ("g_padded_x_expanded_gx_transposed", "padded", "expanded", "transposed")]

Case = namedtuple("Case", "form dt width pairing shape")


def pairing_rows(p):
    return max(rows_of(name) for name in p[1:])


def cases(form):
    """every (width, pairing) the GPU tier runs for a launch form, with the launch shape the width selects:
    fwd / fwd_ac1 (by_reg_shape: width = nvec at the top of the rung, shape = that nvec), fwd_wide (width = nh, shape = (TPR, HPT)),
    bwd_mask / bwd_wide / bwd_rows (shape = vectors or half-vectors per thread)"""
    out = []
    if form in ("fwd", "fwd_ac1"):
        for dt in (("bf16", "fp16", "fp32") if form == "fwd" else ("bf16", "fp16")):
            out += [Case(form, dt, n, p, n - 1) for n in NVECS for p in PAIRINGS]
    elif form == "fwd_wide":
        for dt in ("bf16", "fp16"):
            out += [Case(form, dt, nh, p, wide_shape(nh)) for nh in WIDE_NH for p in PAIRINGS + [HALF_SRC]]
    elif form == "bwd_mask":
        for dt in ("bf16", "fp16", "fp32"):
            out += [Case(form, dt, n, p, backward_vpt(n - 1)) for n in MASK_BWD_NVECS for p in PAIRINGS]
    elif form == "bwd_wide":
        for dt in ("bf16", "fp16"):
            out += [Case(form, dt, nh, p, (nh + 255) // 256) for nh in WIDE_BWD_NH for p in PAIRINGS + [HALF_DST]]
    elif form == "bwd_rows":
        for dt in ("bf16", "fp16", "fp32"):
            out += [Case(form, dt, n, t, rows_vpt(n)) for n in ROW_NVECS for t in TRIPLES]
    else:
        raise KeyError(form)
    return out


FORMS = ("fwd", "fwd_ac1", "fwd_wide", "bwd_mask", "bwd_wide", "bwd_rows")


def case_cols(c):
    """elements per row of a case"""
    if c.form in ("fwd_wide", "bwd_wide"):
        return c.width * 4
    return (c.width if c.form == "bwd_rows" else c.width - 1) * C.EPV[c.dt]


def case_epvs(c):
    """-> (elements per 16-byte vector of the source, of the destination): the fp32-result forward writes fp32, the fp32-gradient backward
    reads it"""
    e = C.EPV[c.dt]
    return (e, 4) if c.form == "fwd_wide" else (4, e) if c.form == "bwd_wide" else (e, e)
