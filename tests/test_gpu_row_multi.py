"""The multi-tensor Sym forward (fq_sym_fwd_pair, fq_sym_fwd_multi with 2 and 4 tensors: the "which tensor of the launch" branch chain of
row_reg_kernel and row_reg_wide_kernel) and the debug forwards (DBG = true: fq_sym_fwd_debug, fq_asym_fwd_debug) on contiguous rows at
every launch shape, on the MI355X.  Tensors of 5, 3, 4 and 1 rows: on the 64-thread rungs one workgroup holds rows of two or three
tensors and the last one is partly empty; bit widths 4 and 8; bounds and bitmap asked of some slots only.  Zero tolerance on bits, any NaN
equals any NaN, every element compared; references: the CPU oracle on each tensor alone, the clip predicate on x for the bitmaps.
The loop is tests/row_ntl_worker.py multi_forward(), which the non-temporal-load worker runs once more (bf16, modes 0 and 2)."""
import numpy as np
import pytest
import torch

import group_cases as C
import row_ntl_worker as W
import row_view_cases as V
from group_ntl_worker import DEV, DTS, from_dev, report, to_dev
from row_ntl_worker import none_failed

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


@pytest.mark.parametrize("dt,mode", [("bf16", 0), ("bf16", 1), ("fp16", 0), ("fp16", 1), ("fp32", 0)])
def test_pair_and_multi_forward_at_every_rung(dt, mode):
    """mode 0: the plain arithmetic, 1: the autocast arithmetic rounded to the tensor dtype; 18 widths x {pair, 2, 4 tensors} = 54 launches"""
    none_failed(W.multi_forward(dt, mode))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_pair_and_multi_forward_at_every_half_vector_count(dt):
    """mode 2, the fp32 result: 20 widths x {pair, 2, 4 tensors} = 60 launches"""
    none_failed(W.multi_forward(dt, 2))


@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_debug_forward_at_every_rung(dt, kind):
    """row_reg_kernel<.., DBG = true>: y, the bin index of every element and the row's scale terms against the oracle's; 18 launches"""
    from llm_qat_amd import _lib
    L = _lib.lib()
    code = {"bf16": _lib.DTYPE_BF16, "fp16": _lib.DTYPE_F16, "fp32": _lib.DTYPE_F32}[dt]
    fn = L.fq_sym_fwd_debug if kind == "sym" else L.fq_asym_fwd_debug
    st = torch.cuda.current_stream().cuda_stream
    failures = []
    for nvec in V.NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        x = to_dev(V.row_bits(dt, cols), dt)
        y = torch.empty(V.ROWS, cols, dtype=DTS[dt], device=DEV)
        idx = torch.full((V.ROWS, cols), 77, dtype=torch.int32, device=DEV)
        scale = torch.full((V.ROWS,) if kind == "sym" else (V.ROWS, 2), 77.0, dtype=torch.float32, device=DEV)
        what = f"{dt} {kind} nvec {nvec} debug"
        rc = fn(x.data_ptr(), y.data_ptr(), idx.data_ptr(), scale.data_ptr(), V.ROWS, cols, V.BITS, code, _lib.SEM_CPU_EAGER, None, 0, st)
        if rc:
            failures.append(f"{what}: refused with code {rc}: {L.fq_last_error().decode(errors='replace')}")
            continue
        want_y, want_idx, want_scale = V.debug_reference(dt, kind, cols)
        failures.append(report(from_dev(y, dt), want_y, dt, what))
        got_idx = idx.cpu().numpy()
        if not np.array_equal(got_idx, want_idx):
            bad = np.argwhere(got_idx != want_idx)
            failures.append(f"{what}: {len(bad)} bin indices differ, first at {bad[:4].tolist()} got {[int(got_idx[tuple(i)]) for i in bad[:4]]} "
                            f"want {[int(want_idx[tuple(i)]) for i in bad[:4]]}")
        failures.append(report(from_dev(scale, "fp32"), want_scale, "fp32", what + " scales"))
    none_failed(failures)
