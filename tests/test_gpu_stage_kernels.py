"""Three kernel families that share the load, statistics and side-output stages of fq_device.h with the register kernels but are not
walked shape by shape in test_gpu_row_launch_shapes.py: the x-reading backwards (fq_ste_bwd_rows at every vectors-per-thread count and
with a short second chunk, fq_ste_bwd), the two-pass path at the smallest row of its vector arm and of its scalar arm, and the
scalar-load kernel at widths around one vector.  Zero tolerance on bits, any NaN equals any NaN, every element compared.  References: the
CPU oracle for the forwards, the clip predicate on x for the backwards, the row's max / min for the bounds."""
import numpy as np
import pytest
import torch

import group_cases as C
import row_ntl_worker as W
from group_ntl_worker import from_dev, report, to_dev
from mx_reference import encode
from row_view_cases import BITS, ROWS, memo, row_bits
from row_ntl_worker import none_failed

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


# ---- the x-reading backward (the loops live in row_ntl_worker.py, which runs them once more with non-temporal loads) --------------------

@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_rows_backward_at_every_vector_count_and_a_short_chunk(dt):
    """5 rows: rows 0 / 2 / 4 can clip (row 2 holds a NaN: its bounds are NaN, its NaN passes the gradient), rows 1 / 3 are copied
    without their x being read"""
    none_failed(W.rows_backward(dt))


@pytest.mark.parametrize("nvec", [257, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_flat_backward(dt, nvec):
    """fq_ste_bwd on n = 257 vectors (two blocks, the second holds one vector) and on a single vector"""
    none_failed(W.flat_backward(dt, nvec))


# ---- the two-pass path -------------------------------------------------------------------------------------------------------------------

# vector arm: the first row length past the register kernels, 8193 vectors = nine chunks of 1024 vectors, the last one a single vector;
# scalar arm: the first width past the scalar-load kernel, nine chunks of 4096 elements, the last one a single element
TWO_PASS = [("bf16", 65544), ("fp32", 32772), ("bf16", 32769), ("fp32", 32769)]


@memo
def two_pass_bits(dt, cols):
    """2 rows; row 1 holds a NaN in its last element (the last chunk of either arm)"""
    b = row_bits(dt, cols, 2).copy()
    b[1, cols - 1] = C.NAN[dt]
    return b


@memo
def two_pass_reference(dt, kind, cols):
    from oracle import oracle as O
    fn = O.sym_fwd if kind == "sym" else O.asym_fwd
    return fn(C.oracle_view(two_pass_bits(dt, cols), dt), 2, cols, BITS, dt, sem=0, want_idx=False)[0].view(C.uint_of(dt)).reshape(2, cols)


@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt,cols", TWO_PASS)
def test_two_pass_at_the_smallest_row_of_each_arm(dt, cols, kind):
    from llm_qat_amd import ops
    b = two_pass_bits(dt, cols)
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    y, bounds = fn(to_dev(b, dt), BITS, want_bounds=True)
    failures = [report(from_dev(y, dt), two_pass_reference(dt, kind, cols), dt, f"{dt} {kind} cols {cols}"),
                report(from_dev(bounds, "fp32"), C.row_bounds(b, dt, kind == "asym").view(np.uint32), "fp32", f"{dt} {kind} cols {cols} bounds")]
    none_failed(failures)


# ---- the scalar-load kernel ---------------------------------------------------------------------------------------------------------------

def generic_cols(dt):
    return [1, C.EPV[dt] - 1, C.EPV[dt] + 1, 257]


@memo
def generic_bits(dt, cols):
    """row_bits for widths that hold its planted values; below that the same rows without them: even rows cross the clip, odd rows stay
    inside it, row 2 ends in a NaN"""
    if cols >= 8:
        return row_bits(dt, cols)
    rng = np.random.default_rng(cols * 7 + ROWS)
    v = rng.standard_normal((ROWS, cols)) * np.where(np.arange(ROWS) % 2 == 0, 1.5, 0.25)[:, None]
    b = encode(v.astype(np.float32).astype(np.float64), dt).astype(C.uint_of(dt))
    b[2, cols - 1] = C.NAN[dt]
    return b


@memo
def generic_reference(dt, kind, cols):
    from oracle import oracle as O
    fn = O.sym_fwd if kind == "sym" else O.asym_fwd
    return fn(C.oracle_view(generic_bits(dt, cols), dt), ROWS, cols, BITS, dt, sem=0, want_idx=False)[0].view(C.uint_of(dt)).reshape(ROWS, cols)


@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_generic_kernel_around_one_vector(dt, kind):
    from llm_qat_amd import ops
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    for cols in generic_cols(dt):
        b = generic_bits(dt, cols)
        y, bounds = fn(to_dev(b, dt), BITS, want_bounds=True)
        failures.append(report(from_dev(y, dt), generic_reference(dt, kind, cols), dt, f"{dt} {kind} cols {cols}"))
        failures.append(report(from_dev(bounds, "fp32"), C.row_bounds(b, dt, kind == "asym").view(np.uint32), "fp32", f"{dt} {kind} cols {cols} bounds"))
    none_failed(failures)
