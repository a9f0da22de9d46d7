"""The pitched instantiations of the row kernels (PITCH = true: the `_v` entry points of ABI 5) at every launch shape, on the MI355X:
row_reg_kernel<.., AC = 0 or 1, PITCH>, row_reg_wide_kernel<.., true, PITCH>, ste_mask_kernel<V, false, true, true>,
ste_mask_wide_kernel<.., true> and ste_rows_kernel<V, false, true, true>.  The launches go through _lib.lib() directly, so the
destination's view is the test's (ops._strided_out would make it contiguous).  Zero tolerance on bits, any NaN equals any NaN, every
element compared, and every element of a destination buffer that no row addresses must still hold its canary.

Widths, layouts, pairings and expected values: tests/row_view_cases.py (the CPU oracle for the forwards, the clip predicate on x for
the bitmaps and the backwards).  tests/test_row_view_cases_cpu.py proves on the CPU that these cases reach every launch shape with every
pairing and see addressing faults.  A failure names the width, the pairing and [row, column] of the first differing elements."""
import numpy as np
import pytest
import torch

import group_cases as C
import row_view_cases as V
from group_ntl_worker import DEV, DTS, from_dev, report, to_dev
from row_ntl_worker import none_failed
from row_view_cases import BITS, HI, LO

pytestmark = pytest.mark.gpu
ESIZE = {"bf16": 2, "fp16": 2, "fp32": 4}
SIDE_FILL = 0xA5


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


def abi():
    from llm_qat_amd import _lib
    return _lib, _lib.lib(), torch.cuda.current_stream().cuda_stream


def code_of(dt):
    from llm_qat_amd import _lib
    return {"bf16": _lib.DTYPE_BF16, "fp16": _lib.DTYPE_F16, "fp32": _lib.DTYPE_F32}[dt]


def rv(view):
    from llm_qat_amd import _lib
    return _lib.RowsView(view.n_inner, view.stride_outer, view.stride_inner)


def at(t, view, dt):
    """the base pointer of a view into buffer t"""
    return t.data_ptr() + view.offset * ESIZE[dt]


def canaries(view, rows, cols, dt):
    n = V.buffer_elems(view, rows, cols) + V.GUARD
    return torch.full((n,), V.CANARY[dt], dtype=torch.int32 if dt == "fp32" else torch.int16, device=DEV).view(DTS[dt])


def check_dest(buf, view, want, dt, what):
    """the rows of a destination buffer against `want`, the rest of it against the canary -> failure texts"""
    got = from_dev(buf, dt)
    rows, cols = want.shape
    out = [report(V.gather(got, view, rows, cols), want, dt, what)]
    rest = ~V.addressed(view, rows, cols, got.size)
    touched = np.flatnonzero(rest & (got != V.CANARY[dt]))
    if touched.size:
        out.append(f"{what}: {touched.size} elements outside the rows were written, first at {touched[:4].tolist()} "
                   f"(row starts {V.row_starts(view, rows, cols).tolist()}, cols {cols})")
    return out


def check_side(side, dt, asym, cols, rows, sv, what):
    """bounds and the bitmap rows of clippable rows of a side buffer, for a source in view sv"""
    want_b, clippable, pred = V.side_expected(dt, asym, cols, rows)
    want_b, clippable, pred = V.as_addressed(want_b, sv), V.as_addressed(clippable, sv), V.as_addressed(pred, sv)
    raw = side.cpu().numpy()
    out = [report(raw[: rows * 8].view(np.uint32).reshape(rows, 2), want_b, "fp32", f"{what} bounds")]
    m = raw[rows * 8:].reshape(rows, -1)
    assert m.shape[1] == V.mask_row_bytes(cols)
    got = np.unpackbits(m, axis=1, bitorder="little")[:, :cols].astype(bool)
    if not np.array_equal(got[clippable], pred[clippable]):
        out.append(f"{what} bitmap differs from the predicate at {np.argwhere(got[clippable] != pred[clippable])[:4].tolist()}")
    return out


def new_side(rows, cols):
    return torch.full((rows * 8 + rows * V.mask_row_bytes(cols),), SIDE_FILL, dtype=torch.uint8, device=DEV)


def refused(L, rc, what):
    return f"{what}: refused with code {rc}: {L.fq_last_error().decode(errors='replace')}"


# ---- forward ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_forward_plain_and_training_at_every_rung_and_pairing(dt, kind):
    """fq_rowwise_fwd_v: 18 widths x 6 pairings x {plain, training} = 216 launches"""
    _lib, L, st = abi()
    code, epv, asym = code_of(dt), C.EPV[dt], kind == "asym"
    failures = []
    for nvec in V.NVECS:
        cols = (nvec - 1) * epv
        for pname, s, d in V.PAIRINGS:
            rows = V.pairing_rows((pname, s, d))
            sv, dv = V.layout(s, cols, epv, rows), V.layout(d, cols, epv, rows)
            x = to_dev(V.source_buffer(V.row_bits(dt, cols, rows), sv, dt)[0], dt)
            want = V.as_addressed(V.forward_reference(dt, kind, cols, rows), sv)
            for train in (False, True):
                what = f"{dt} {kind} nvec {nvec} {pname} {'training' if train else 'plain'}"
                y = canaries(dv, rows, cols, dt)
                side = new_side(rows, cols)
                sp = side.data_ptr()
                rc = L.fq_rowwise_fwd_v(int(asym), at(x, sv, dt), rv(sv), at(y, dv, dt), rv(dv), rows, cols, BITS, code, _lib.SEM_CPU_EAGER, LO, HI,
                                        sp if train else None, sp + rows * 8 if train else None, rows * V.mask_row_bytes(cols) if train else 0, st)
                if rc:
                    failures.append(refused(L, rc, what))
                    continue
                failures += check_dest(y, dv, want, dt, what)
                if train:
                    failures += check_side(side, dt, asym, cols, rows, sv, what)
                elif not bool((side == SIDE_FILL).all()):
                    failures.append(f"{what}: a side buffer it was not given was written")
    none_failed(failures)


def autocast_v(dt, mode, widths, pairings):
    """fq_sym_fwd_multi_v with one tensor under the autocast arithmetic (mode 1: the tensor dtype, 2: the fp32 result), plain and training"""
    _lib, L, st = abi()
    code, ydt = code_of(dt), "fp32" if mode == 2 else dt
    failures = []
    for wname, cols in widths:
        for pname, s, d in pairings:
            rows = V.pairing_rows((pname, s, d))
            sv, dv = V.layout(s, cols, 8, rows), V.layout(d, cols, C.EPV[ydt], rows)
            x = to_dev(V.source_buffer(V.row_bits(dt, cols, rows), sv, dt)[0], dt)
            want = V.as_addressed(V.autocast_reference(dt, mode == 2, cols, rows), sv)
            for train in (False, True):
                what = f"{dt} autocast {mode} {wname} {pname} {'training' if train else 'plain'}"
                y = canaries(dv, rows, cols, ydt)
                side = new_side(rows, cols)
                sp = side.data_ptr()
                t = (_lib.FwdTensorV * 1)(_lib.FwdTensorV(at(x, sv, dt), at(y, dv, ydt), rows, BITS, sp if train else None, sp + rows * 8 if train else None,
                                                          rows * V.mask_row_bytes(cols) if train else 0, rv(sv), rv(dv)))
                rc = L.fq_sym_fwd_multi_v(1, t, cols, code, _lib.SEM_DEVICE_EAGER, mode, LO, HI, st)
                if rc:
                    failures.append(refused(L, rc, what))
                    continue
                failures += check_dest(y, dv, want, ydt, what)
                if train:
                    failures += check_side(side, dt, False, cols, rows, sv, what)
                elif not bool((side == SIDE_FILL).all()):
                    failures.append(f"{what}: a side buffer it was not given was written")
    return failures


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_narrow_at_every_rung_and_pairing(dt):
    """row_reg_kernel<.., AC = 1, PITCH>: 18 widths x 6 pairings x 2 = 216 launches"""
    none_failed(autocast_v(dt, 1, [(f"nvec {n}", (n - 1) * 8) for n in V.NVECS], V.PAIRINGS))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_wide_at_every_half_vector_count_and_pairing(dt):
    """row_reg_wide_kernel<.., true, PITCH> (the one flavour pitched rows have, with and without a bitmap to record): 20 widths x 7
    pairings -- the seventh is the source whose rows are 8-byte but not 16-byte aligned -- x 2 = 280 launches"""
    none_failed(autocast_v(dt, 2, [(f"nh {nh}", nh * 4) for nh in V.WIDE_NH], V.PAIRINGS + [V.HALF_SRC]))


# ---- backward from (bounds, bitmap) -------------------------------------------------------------------------------------------------------

def masked(g_rows, dt, cols, rows):
    """the gradient rows as addressed, with +0.0 where row r's predicate holds (bounds and bitmap are indexed by the row number)"""
    want = g_rows.copy()
    want[V.side_expected(dt, False, cols, rows)[2]] = 0
    return want


def bwd_tensor(_lib, g, gv, gdt, gx, gxv, xdt, rows, side):
    return _lib.BwdTensorV(at(g, gv, gdt), at(gx, gxv, xdt), rows, side.data_ptr(), side.data_ptr() + rows * 8, rv(gv), rv(gxv))


def mask_backward_v(dt, wide):
    """fq_ste_bwd_mask_multi_v at every (half-)vector count: one copying tensor in every pairing, two tensors of which one is pitched,
    and (16-bit or fp32 gradients of the tensor's own dtype only) one tensor in place in every pitched layout.  The side buffers are built
    from the predicate; the bitmap rows of unclippable rows hold junk the backward must not read."""
    _lib, L, st = abi()
    code = code_of(dt)
    gdt = "fp32" if wide else dt
    ge, xe = C.EPV[gdt], C.EPV[dt]
    widths = [(f"nh {nh}", nh * 4) for nh in V.WIDE_BWD_NH] if wide else [(f"nvec {n}", (n - 1) * xe) for n in V.MASK_BWD_NVECS]
    pairings = V.PAIRINGS + ([V.HALF_DST] if wide else [])
    failures = []

    def grads(cols, rows, gv):
        g, cast = V.wide_grad_and_cast(dt, cols, rows) if wide else (V.grad_and_masked(dt, cols, rows)[0],) * 2
        buf, _ = V.source_buffer(g, gv, gdt)
        return to_dev(buf, gdt), buf, masked(V.as_addressed(cast, gv), dt, cols, rows)

    for wname, cols in widths:
        g5, _, want5 = grads(cols, V.ROWS, V.CONTIG)
        side5 = torch.from_numpy(V.side_bytes(dt, False, cols, V.ROWS)).to(DEV)
        for i, (pname, s, d) in enumerate(pairings):
            rows = V.pairing_rows((pname, s, d))
            gv, ov = V.layout(s, cols, ge, rows), V.layout(d, cols, xe, rows)
            g, _, want = grads(cols, rows, gv)
            side = torch.from_numpy(V.side_bytes(dt, False, cols, rows)).to(DEV)
            what = f"{dt} {'fp32-gradient ' if wide else ''}backward {wname} {pname}"
            gx = canaries(ov, rows, cols, dt)
            rc = L.fq_ste_bwd_mask_multi_v(1, (_lib.BwdTensorV * 1)(bwd_tensor(_lib, g, gv, gdt, gx, ov, dt, rows, side)), cols, LO, HI, code, int(wide), st)
            failures += [refused(L, rc, what)] if rc else check_dest(gx, ov, want, dt, what)
            # two tensors, one of them pitched: alternately the second and the first
            gx, gx5 = canaries(ov, rows, cols, dt), canaries(V.CONTIG, V.ROWS, cols, dt)
            pair = [bwd_tensor(_lib, g5, V.CONTIG, gdt, gx5, V.CONTIG, dt, V.ROWS, side5), bwd_tensor(_lib, g, gv, gdt, gx, ov, dt, rows, side)]
            rc = L.fq_ste_bwd_mask_multi_v(2, (_lib.BwdTensorV * 2)(*(pair if i % 2 == 0 else pair[::-1])), cols, LO, HI, code, int(wide), st)
            what += f", {'second' if i % 2 == 0 else 'first'} of two tensors"
            failures += [refused(L, rc, what)] if rc else check_dest(gx, ov, want, dt, what) + check_dest(gx5, V.CONTIG, want5, dt, what + ": the contiguous one")
        if wide:
            continue
        for name in V.INPLACE_LAYOUTS:
            rows = V.rows_of(name)
            v = V.layout(name, cols, xe, rows)
            g, buf, want = grads(cols, rows, v)
            side = torch.from_numpy(V.side_bytes(dt, False, cols, rows)).to(DEV)
            rc = L.fq_ste_bwd_mask_multi_v(1, (_lib.BwdTensorV * 1)(bwd_tensor(_lib, g, v, dt, g, v, dt, rows, side)), cols, LO, HI, code, 0, st)
            what = f"{dt} backward {wname} in place in {name}"
            if rc:
                failures.append(refused(L, rc, what))
                continue
            left = buf.copy()           # what stood between the rows must still stand there
            for r, s0 in enumerate(V.row_starts(v, rows, cols)):
                left[s0: s0 + cols] = want[r]
            failures.append(report(from_dev(g, dt), left, dt, what))
    return failures


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_mask_backward_at_every_vector_count_and_pairing(dt):
    """ste_mask_kernel<V, false, true, true>: 8 widths x (6 pairings x 2 + 4 in place) = 128 launches"""
    none_failed(mask_backward_v(dt, False))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wide_mask_backward_at_every_half_vector_count_and_pairing(dt):
    """ste_mask_wide_kernel<.., true>: 8 widths x 7 pairings -- the seventh is the gx whose rows are 8-byte but not 16-byte aligned --
    x 2 = 112 launches"""
    none_failed(mask_backward_v(dt, True))


# ---- the x-reading backward ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_rows_backward_with_three_views(dt):
    """fq_ste_bwd_v (ste_rows_kernel<V, false, true, true>) at 256 v - 1 and 2049 vectors, g, x and gx each in a view of its own, with
    and without row bounds: 9 widths x 4 triples x 2 = 72 launches"""
    _lib, L, st = abi()
    code, epv = code_of(dt), C.EPV[dt]
    failures = []
    for nvec in V.ROW_NVECS:
        cols = nvec * epv
        for tname, gn, xn, on in V.TRIPLES:
            rows = V.pairing_rows((tname, gn, xn, on))
            gv, xv, ov = (V.layout(n, cols, epv, rows) for n in (gn, xn, on))
            gbuf, g_rows = V.source_buffer(V.grad_and_masked(dt, cols, rows)[0], gv, dt)
            xbuf, x_rows = V.source_buffer(V.row_bits(dt, cols, rows), xv, dt)
            want = g_rows.copy()
            want[C.clip_predicate(x_rows, dt, LO, HI)] = 0
            g, x = to_dev(gbuf, dt), to_dev(xbuf, dt)
            bounds = torch.from_numpy(C.row_bounds(x_rows, dt, False)).to(DEV)
            for b in (None, bounds):
                what = f"{dt} nvec {nvec} rows backward {tname} {'with' if b is not None else 'without'} bounds"
                gx = canaries(ov, rows, cols, dt)
                rc = L.fq_ste_bwd_v(at(g, gv, dt), rv(gv), at(x, xv, dt), rv(xv), at(gx, ov, dt), rv(ov), rows, cols, LO, HI,
                                    b.data_ptr() if b is not None else None, code, st)
                failures += [refused(L, rc, what)] if rc else check_dest(gx, ov, want, dt, what)
    none_failed(failures)


# ---- two tensors in one forward launch, the second one pitched ------------------------------------------------------------------------------

PAIR_NVECS = [64, 128, 192, 3072, 8192]        # the three 64-thread rungs (one workgroup holds rows of both tensors), 512 x 6, 1024 x 8
PAIR_NH = [62, 126, 510, 2046, 8190]


@pytest.mark.parametrize("dt,mode", [("bf16", 0), ("bf16", 1), ("bf16", 2), ("fp16", 0), ("fp16", 1), ("fp16", 2), ("fp32", 0)])
def test_two_tensor_forward_with_the_second_one_pitched(dt, mode):
    """fq_sym_fwd_multi_v, tensors of 5 (contiguous, 4 bits) and 3 rows (a slice stored into every other row, 8 bits), both recording:
    5 launches per (dtype, arithmetic)"""
    _lib, L, st = abi()
    code, ydt = code_of(dt), "fp32" if mode == 2 else dt
    sem = _lib.SEM_DEVICE_EAGER if mode else _lib.SEM_CPU_EAGER
    failures = []
    for wname, cols in ([(f"nh {nh}", nh * 4) for nh in PAIR_NH] if mode == 2 else [(f"nvec {n}", (n - 1) * C.EPV[dt]) for n in PAIR_NVECS]):
        sv, dv = V.layout("slice", cols, C.EPV[dt], 3), V.layout("every_other", cols, C.EPV[ydt], 3)
        x5 = to_dev(V.row_bits(dt, cols, 5), dt)
        x3 = to_dev(V.source_buffer(V.row_bits(dt, cols, 3), sv, dt)[0], dt)
        y5, y3 = canaries(V.CONTIG, 5, cols, ydt), canaries(dv, 3, cols, ydt)
        s5, s3 = new_side(5, cols), new_side(3, cols)
        t = (_lib.FwdTensorV * 2)(
            _lib.FwdTensorV(x5.data_ptr(), y5.data_ptr(), 5, 4, s5.data_ptr(), s5.data_ptr() + 40, 5 * V.mask_row_bytes(cols), rv(V.CONTIG), rv(V.CONTIG)),
            _lib.FwdTensorV(at(x3, sv, dt), at(y3, dv, ydt), 3, 8, s3.data_ptr(), s3.data_ptr() + 24, 3 * V.mask_row_bytes(cols), rv(sv), rv(dv)))
        rc = L.fq_sym_fwd_multi_v(2, t, cols, code, sem, mode, LO, HI, st)
        what = f"{dt} mode {mode} {wname}"
        if rc:
            failures.append(refused(L, rc, what))
            continue
        failures += check_dest(y5, V.CONTIG, V.sym_reference(dt, mode, cols, 5, 4), ydt, what + " contiguous slot")
        failures += check_dest(y3, dv, V.sym_reference(dt, mode, cols, 3, 8), ydt, what + " pitched slot")
        failures += check_side(s5, dt, False, cols, 5, V.CONTIG, what + " contiguous slot") + check_side(s3, dt, False, cols, 3, sv, what + " pitched slot")
    none_failed(failures)
