"""Three kernel families that share the load, statistics and side-output stages of fq_device.h with the register kernels but are not
walked shape by shape in test_gpu_row_launch_shapes.py: the x-reading backwards (fq_ste_bwd_rows at every vectors-per-thread count and
with a short second chunk, fq_ste_bwd), the two-pass path at the smallest row of its vector arm and of its scalar arm, and the
scalar-load kernel at widths around one vector.  Zero tolerance on bits, any NaN equals any NaN, every element compared.  References: the
CPU oracle for the forwards, the clip predicate on x for the backwards, the row's max / min for the bounds."""
import numpy as np
import pytest
import torch

import group_cases as C
from group_ntl_worker import from_dev, report, to_dev
from mx_reference import encode
from test_gpu_row_launch_shapes import BITS, HI, LO, ROWS, grad_and_masked, memo, none_failed, row_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


def dev_bounds(bits, dt, asym=False):
    return torch.from_numpy(C.row_bounds(bits, dt, asym)).to("cuda")


# ---- the x-reading backward --------------------------------------------------------------------------------------------------------------

# rows of 256 v - 1 vectors: v vectors per thread (launch_ste_rows), the last lane slot a clamped duplicate; 2049 vectors: two chunks of
# 1025 and 1024 vectors at 5 vectors per thread, the second one short
ROW_NVECS = [256 * v - 1 for v in range(1, 9)] + [2049]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_rows_backward_at_every_vector_count_and_a_short_chunk(dt):
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
        got = ops.ste_backward(to_dev(g, dt), to_dev(b, dt), LO, HI, row_bounds=dev_bounds(b, dt), rows_cols_hint=(ROWS, cols))
        failures.append(report(from_dev(got, dt), want, dt, f"{dt} nvec {nvec} rows backward"))
    none_failed(failures)


@pytest.mark.parametrize("nvec", [257, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_flat_backward(dt, nvec):
    """fq_ste_bwd on n = 257 vectors (two blocks, the second holds one vector) and on a single vector"""
    from llm_qat_amd import ops
    cols = nvec * C.EPV[dt]
    g, want = grad_and_masked(dt, cols, 1)
    assert want.any() and (want != g).any()
    got = ops.ste_backward(to_dev(g, dt), to_dev(row_bits(dt, cols, 1), dt), LO, HI)
    assert report(from_dev(got, dt), want, dt, f"{dt} {nvec} vectors flat backward") is None


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
