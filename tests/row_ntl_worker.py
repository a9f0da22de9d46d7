"""The loops of the row kernels' launch-shape walk (tests/test_gpu_row_launch_shapes.py), of the x-reading and flat backwards
(tests/test_gpu_stage_kernels.py) and of the multi-tensor forward (tests/test_gpu_row_multi.py), as functions that return failure texts.
The test files call them in their own process, where no tensor of the walk is large enough for the non-temporal loads, and start this
file as a program in a FRESH child interpreter with LLMQAT_FQ_NT_LOAD_MIN_MB=0 (the library reads that variable once per process),
where every launch of the walk takes the streamed instantiation: the Sym forward with `nt sc1` stores, the ntl forms of the autocast
forwards, ste_mask_one_kernel<V, true>, the two-slot ste_mask_kernel<V, true, ST_NT_SC1, false, 2>, the four-slot ste_mask_kernel<V, true>,
the ntl ste_mask_wide_kernel (always its four-slot form), ste_rows_kernel<V, true> and ste_vec_kernel<1, true>.

    LLMQAT_FQ_NT_LOAD_MIN_MB=0 python tests/row_ntl_worker.py <out.json>

Test infrastructure: writes {"cases": launches, "failures": [...]} and exits non-zero if any result differs from its reference.
Zero tolerance on bits, any NaN equals any NaN, every element compared."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import group_cases as C  # noqa: E402
from group_ntl_worker import DEV, DTS, from_dev, report, to_dev  # noqa: E402
from row_view_cases import (BITS, HI, LO, NVECS, ROW_NVECS, ROWS, WIDE_BWD_NH, WIDE_NH, autocast_reference, forward_reference,  # noqa: E402
                            grad_and_masked, mask_row_bytes, row_bits, side_expected, side_reference, sym_reference, wide_grad_and_masked)

launches = [0]


def launch(fn, *args, **kw):
    """fn(*args, **kw), counted: every call is one kernel launch of the walk"""
    launches[0] += 1
    return fn(*args, **kw)


def unpack_mask(mask, rows, cols):
    m = mask.cpu().numpy().reshape(rows, -1)
    assert m.shape[1] == (cols + 63) // 64 * 8
    return np.unpackbits(m, axis=1, bitorder="little")[:, :cols].astype(bool)


def split(side, rows):
    return side[: rows * 8].view(torch.float32).view(rows, 2), side[rows * 8:]


def check_side(bounds, mask, dt, asym, cols, what, rows=ROWS):
    want_b, clippable, pred = side_reference(dt, asym, cols, rows)
    out = [report(from_dev(bounds, "fp32"), want_b, "fp32", f"{what} bounds")]
    got = unpack_mask(mask, rows, cols)
    if not np.array_equal(got[clippable], pred[clippable]):
        out.append(f"{what} bitmap differs from the predicate at {np.argwhere(got[clippable] != pred[clippable])[:4].tolist()}")
    return out


def none_failed(failures):
    failures = [f for f in failures if f]
    assert not failures, (len(failures), failures[:5])


# ---- forward: every rung of the register ladder ---------------------------------------------------------------------------------------------

def forward_plain_and_training(dt, kind):
    from llm_qat_amd import ops
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        x = to_dev(row_bits(dt, cols), dt)
        want = forward_reference(dt, kind, cols)
        failures.append(report(from_dev(launch(fn, x, BITS), dt), want, dt, f"{dt} {kind} nvec {nvec} plain"))
        res = launch(ops.quantize_train, kind, x, BITS, False, LO, HI)
        assert res is not None, (dt, kind, nvec)
        y, bounds, mask = res
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} {kind} nvec {nvec} training"))
        failures += check_side(bounds, mask, dt, kind == "asym", cols, f"{dt} {kind} nvec {nvec}")
    return failures


def autocast_narrow(dt):
    from llm_qat_amd import ops
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        x = to_dev(row_bits(dt, cols), dt)
        want = autocast_reference(dt, False, cols)
        y = launch(ops.sym_forward_autocast, x, BITS, False, wide=False)[0]
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} autocast nvec {nvec} plain"))
        y, side, rows, _, got = launch(ops.sym_forward_autocast, x, BITS, False, wide=False, lo=LO, hi=HI, train="mask")
        assert got == "mask" and rows == ROWS, (dt, nvec, got)
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} autocast nvec {nvec} training"))
        failures += check_side(*split(side, ROWS), dt, False, cols, f"{dt} autocast nvec {nvec}")
    return failures


def autocast_wide(dt):
    from llm_qat_amd import ops
    failures = []
    for nh in WIDE_NH + WIDE_BWD_NH[:2]:
        cols = nh * 4
        x = to_dev(row_bits(dt, cols), dt)
        want = autocast_reference(dt, True, cols)
        y = launch(ops.sym_forward_autocast, x, BITS, False, wide=True)[0]
        assert y.dtype is torch.float32
        failures.append(report(from_dev(y, "fp32"), want, "fp32", f"{dt} wide nh {nh} plain"))
        y, side, _, _, got = launch(ops.sym_forward_autocast, x, BITS, False, wide=True, lo=LO, hi=HI, train="mask")
        assert got == "mask", (dt, nh, got)
        failures.append(report(from_dev(y, "fp32"), want, "fp32", f"{dt} wide nh {nh} training"))
        failures += check_side(*split(side, ROWS), dt, False, cols, f"{dt} wide nh {nh}")
        # the fp32-gradient backward on that forward's side outputs: one slot, and two slots with a 3-row tensor of the same width
        g, want_g = wide_grad_and_masked(dt, cols)
        gout = to_dev(g, "fp32")
        failures.append(report(from_dev(launch(ops.train_backward_wide, gout, side, ROWS, cols, LO, HI, DTS[dt]), dt), want_g, dt, f"{dt} wide nh {nh} backward"))
        if nh in WIDE_BWD_NH:
            x3 = to_dev(row_bits(dt, cols, 3), dt)
            side3 = launch(ops.sym_forward_autocast, x3, BITS, False, wide=True, lo=LO, hi=HI, train="mask")[1]
            g3, want_g3 = wide_grad_and_masked(dt, cols, 3)
            o5, o3 = launch(ops.pair_backward_wide, gout, to_dev(g3, "fp32"), side, side3, ROWS, 3, cols, LO, HI, DTS[dt])
            failures.append(report(from_dev(o5, dt), want_g, dt, f"{dt} wide nh {nh} backward, slot 0 of 2"))
            failures.append(report(from_dev(o3, dt), want_g3, dt, f"{dt} wide nh {nh} backward, slot 1 of 2"))
    return failures


# ---- backward from (bounds, bitmap): every vector count in every launch form ---------------------------------------------------------------

def mask_backward_one_tensor_and_in_place(dt, kind):
    from llm_qat_amd import ops
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        _, bounds, mask = launch(ops.quantize_train, kind, to_dev(row_bits(dt, cols), dt), BITS, False, LO, HI)
        g, want = grad_and_masked(dt, cols)
        gout = to_dev(g, dt)
        failures.append(report(from_dev(launch(ops.ste_backward_mask, gout, LO, HI, bounds, mask, ROWS, cols), dt), want, dt, f"{dt} {kind} nvec {nvec} backward"))
        gin = gout.clone()
        out = launch(ops.ste_backward_mask, gin, LO, HI, bounds, mask, ROWS, cols, inplace=True)
        assert out.data_ptr() == gin.data_ptr()
        failures.append(report(from_dev(out, dt), want, dt, f"{dt} {kind} nvec {nvec} backward in place"))
    return failures


def mask_backward_two_and_four_slot_forms(dt):
    """the two-slot form (pair_backward: both copying, and the first slot in place as a weight's gradient is) and the four-slot form
    (multi_backward with three tensors, the first in place): tensors of 5, 3 and 4 rows of the same width"""
    from llm_qat_amd import ops
    failures = []
    nrows = (ROWS, 3, 4)
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        sides = [launch(ops.train_forward, "sym", to_dev(row_bits(dt, cols, r), dt), BITS, False, LO, HI)[1] for r in nrows]
        gw = [grad_and_masked(dt, cols, r) for r in nrows]
        for inplace in (False, True):
            what = f"{dt} nvec {nvec} inplace {inplace}"
            g0, g1, g2 = (to_dev(g, dt) for g, _ in gw)
            o0, o1 = launch(ops.pair_backward, g0, g1, sides[0], sides[1], nrows[0], nrows[1], cols, LO, HI, inplace_w=inplace)
            assert (o0.data_ptr() == g0.data_ptr()) == inplace
            failures.append(report(from_dev(o0, dt), gw[0][1], dt, f"{what} pair slot 0"))
            failures.append(report(from_dev(o1, dt), gw[1][1], dt, f"{what} pair slot 1"))
            g0 = to_dev(gw[0][0], dt)
            outs = launch(ops.multi_backward, [g0, g1, g2], sides, list(nrows), cols, LO, HI, inplace=[inplace, False, False])
            assert (outs[0].data_ptr() == g0.data_ptr()) == inplace
            for i, o in enumerate(outs):
                failures.append(report(from_dev(o, dt), gw[i][1], dt, f"{what} multi slot {i}"))
    return failures


# ---- the x-reading backwards ----------------------------------------------------------------------------------------------------------------

def dev_bounds(bits, dt, asym=False):
    return torch.from_numpy(C.row_bounds(bits, dt, asym)).to("cuda")


def rows_backward(dt):
    """5 rows: rows 0 / 2 / 4 can clip (row 2 holds a NaN: its bounds are NaN, its NaN passes the gradient), rows 1 / 3 are copied
    without their x being read"""
    from llm_qat_amd import ops
    failures = []
    for nvec in ROW_NVECS:
        cols = nvec * C.EPV[dt]
        b = row_bits(dt, cols)
        bounds = C.row_bounds(b, dt, False)
        safe = (bounds[:, 0] < HI) & (bounds[:, 1] > LO)
        assert safe.any() and (~safe).any() and np.isnan(bounds[2]).all()
        g, want = grad_and_masked(dt, cols)
        got = launch(ops.ste_backward, to_dev(g, dt), to_dev(b, dt), LO, HI, row_bounds=dev_bounds(b, dt), rows_cols_hint=(ROWS, cols))
        failures.append(report(from_dev(got, dt), want, dt, f"{dt} nvec {nvec} rows backward"))
    return failures


def flat_backward(dt, nvec):
    """fq_ste_bwd on n = 257 vectors (two blocks, the second holds one vector) and on a single vector"""
    from llm_qat_amd import ops
    cols = nvec * C.EPV[dt]
    g, want = grad_and_masked(dt, cols, 1)
    assert want.any() and (want != g).any()
    got = launch(ops.ste_backward, to_dev(g, dt), to_dev(row_bits(dt, cols, 1), dt), LO, HI)
    return [report(from_dev(got, dt), want, dt, f"{dt} {nvec} vectors flat backward")]


# ---- the multi-tensor Sym forward on contiguous rows: fq_sym_fwd_pair and fq_sym_fwd_multi -----------------------------------------------

MULTI_ROWS = (5, 3, 4, 1)     # 64-thread workgroups (four rows each) straddle the slot boundaries; the last one is partly empty
MULTI_BITS = (4, 8, 8, 4)
MULTI_SIDE = (True, False, True, False)    # which slots ask for bounds + bitmap
SIDE_FILL = 0xA5


def multi_forward(dt, mode, widths=None):
    """fq_sym_fwd_pair and fq_sym_fwd_multi (n = 2 and 4) through the C ABI at every width of the ladder the mode uses (mode 0 / 1: every
    rung of by_reg_shape; 2: every half-vector count of the fp32-result forward): each slot's y, bounds and bitmap against the oracle
    for that tensor alone; the side buffers of slots that asked for none stay as they were filled"""
    from llm_qat_amd import _lib
    L = _lib.lib()
    code = {"bf16": _lib.DTYPE_BF16, "fp16": _lib.DTYPE_F16, "fp32": _lib.DTYPE_F32}[dt]
    ydt = "fp32" if mode == 2 else dt
    sem = _lib.SEM_DEVICE_EAGER if mode else _lib.SEM_CPU_EAGER
    st = torch.cuda.current_stream().cuda_stream
    failures = []
    if widths is None:
        widths = [(f"nh {nh}", nh * 4) for nh in WIDE_NH] if mode == 2 else [(f"nvec {n}", (n - 1) * C.EPV[dt]) for n in NVECS]
    for wname, cols in widths:
        mb = [r * mask_row_bytes(cols) for r in MULTI_ROWS]
        xs = [to_dev(row_bits(dt, cols, r), dt) for r in MULTI_ROWS]
        for form in ("pair", "multi2", "multi4"):
            n = 4 if form == "multi4" else 2
            ys = [torch.empty(r, cols, dtype=DTS[ydt], device=DEV) for r in MULTI_ROWS[:n]]
            sides = [torch.full((r * 8 + mb[i],), SIDE_FILL, dtype=torch.uint8, device=DEV) for i, r in enumerate(MULTI_ROWS[:n])]
            want_side = MULTI_SIDE[:n] if form != "multi2" else MULTI_SIDE[1:3]     # multi2: the SECOND slot records
            t = []
            for i in range(n):
                sp = sides[i].data_ptr()
                t.append((xs[i].data_ptr(), ys[i].data_ptr(), MULTI_ROWS[i], MULTI_BITS[i], sp if want_side[i] else None,
                          sp + MULTI_ROWS[i] * 8 if want_side[i] else None, mb[i] if want_side[i] else 0))
            if form == "pair":
                rc = launch(L.fq_sym_fwd_pair, *t[0], *t[1], cols, code, sem, mode, LO, HI, st)
            else:
                arr = (_lib.FwdTensor * n)(*[_lib.FwdTensor(*f) for f in t])
                rc = launch(L.fq_sym_fwd_multi, n, arr, cols, code, sem, mode, LO, HI, st)
            what = f"{dt} mode {mode} {wname} {form}"
            if rc:
                failures.append(f"{what}: refused with code {rc}: {L.fq_last_error().decode(errors='replace')}")
                continue
            for i in range(n):
                r = MULTI_ROWS[i]
                failures.append(report(from_dev(ys[i], ydt), sym_reference(dt, mode, cols, r, MULTI_BITS[i]), ydt, f"{what} slot {i}"))
                if not want_side[i]:
                    if not bool((sides[i] == SIDE_FILL).all()):
                        failures.append(f"{what} slot {i}: its side buffer was written though it asked for none")
                    continue
                want_b, clippable, pred = side_expected(dt, False, cols, r)
                bounds, mask = split(sides[i], r)
                failures.append(report(from_dev(bounds, "fp32"), want_b, "fp32", f"{what} slot {i} bounds"))
                got = unpack_mask(mask, r, cols)
                if not np.array_equal(got[clippable], pred[clippable]):
                    failures.append(f"{what} slot {i}: bitmap differs from the predicate at {np.argwhere(got[clippable] != pred[clippable])[:4].tolist()}")
    return failures


# ---- the walk of the child interpreter --------------------------------------------------------------------------------------------------

def walk():
    """-> failure texts of every function above on bf16 (and fp32 where the launch form serves it)"""
    import llm_qat_amd
    llm_qat_amd.set_semantics("cpu_eager")
    failures = []
    for dt in ("bf16", "fp32"):
        for kind in ("sym", "asym"):
            failures += forward_plain_and_training(dt, kind)
        failures += mask_backward_one_tensor_and_in_place(dt, "sym")
        failures += mask_backward_two_and_four_slot_forms(dt)
        failures += rows_backward(dt)
        failures += flat_backward(dt, 257) + flat_backward(dt, 1)
    failures += autocast_narrow("bf16") + autocast_wide("bf16")
    failures += multi_forward("bf16", 0) + multi_forward("bf16", 2)
    return [f for f in failures if f]


def walk_launches():
    """the launches walk() makes, from the case lists alone"""
    n, w = len(NVECS), len(WIDE_NH) + 2
    b = sum(nh in WIDE_BWD_NH for nh in WIDE_NH + WIDE_BWD_NH[:2])
    per_dt = 2 * (2 * n) + 3 * n + n * (3 + 2 * 2) + len(ROW_NVECS) + 2
    return 2 * per_dt + 2 * n + (3 * w + 2 * b) + 3 * n + 3 * len(WIDE_NH)


def main(out):
    assert os.environ.get("LLMQAT_FQ_NT_LOAD_MIN_MB") == "0", "start this worker with LLMQAT_FQ_NT_LOAD_MIN_MB=0"
    failures = walk()
    torch.cuda.synchronize()
    with open(out, "w") as fh:
        json.dump({"cases": launches[0], "failures": failures[:20]}, fh)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
