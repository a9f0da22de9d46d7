"""Operands and the float64 reference of the MX GEMM tests.  The reference is ops.MXExport.dequantize() on CPU tensors (plain torch ops,
proved bit for bit against tests/mx_reference.py by test_gpu_mx.py), cast to double, then one matmul: it shares no code with the kernel."""
import numpy as np
import torch

from llm_qat_amd import ops

from mx_reference import pack_fp4

GEMM_FMTS = ["mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"]
PAIRS = [(a, w) for a in GEMM_FMTS for w in GEMM_FMTS]
_F8 = {"mxfp8_e4m3": torch.float8_e4m3fn, "mxfp8_e5m2": torch.float8_e5m2}
FP4_GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)   # magnitudes of the 8 E2M1 codes


def export_from_codes(codes, scales, fmt):
    """codes: uint8 [rows, K] (one element code each: 4-bit for mxfp4, an OCP byte for mxfp8_*); scales: uint8 [rows, K / 32]
    -> a CPU MXExport of dtype float32 in exactly the layout ops.mx_export writes."""
    codes, scales = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(scales, dtype=np.uint8)
    rows, K = codes.shape
    assert scales.shape == (rows, K // 32)
    elems = pack_fp4(codes.reshape(-1)).reshape(rows, K // 2) if fmt == "mxfp4" else codes
    return ops.MXExport(torch.from_numpy(np.ascontiguousarray(elems)), torch.from_numpy(scales), fmt, (rows, K), torch.float32)


def codes_of_values(values, fmt):
    """element codes of values that lie on the FP4 grid (signed multiples of 0.5 up to 6: exact in all three formats)"""
    values = np.asarray(values, dtype=np.float32)
    if fmt == "mxfp4":
        mag = np.abs(values)
        idx = np.searchsorted(FP4_GRID, mag)
        assert np.array_equal(FP4_GRID[idx], mag), "not on the FP4 grid"
        return (idx | (np.signbit(values) << 3)).astype(np.uint8)
    t = torch.from_numpy(values).to(_F8[fmt])
    assert torch.equal(t.float(), torch.from_numpy(values)), "not exact in the fp8 format"
    return t.view(torch.uint8).numpy()


def to_device(e, device="cuda"):
    return ops.MXExport(e.elements.to(device), e.scales.to(device), e.fmt, e.shape, e.dtype)


def to_cpu(e):
    return ops.MXExport(e.elements.cpu(), e.scales.cpu(), e.fmt, e.shape, torch.float32)


def ref64(a, w):
    """a, w: CPU MXExports of dtype float32 (dequantize() is then exact) -> (ref, S) = (A @ W.T, |A| @ |W|.T) in float64"""
    A = a.dequantize().double().reshape(-1, a.shape[-1])
    W = w.dequantize().double()
    return A @ W.T, A.abs() @ W.abs().T


def grid_operand(rng, rows, K, fmt, scale_choices=(127, 128)):
    """random FP4-grid values (so every product is a multiple of 0.25 * the scales) with scales drawn from scale_choices
    -> (CPU MXExport, integer form: values / 0.5 * 2^(scale - min scale) as int64 [rows, K])"""
    mag = rng.integers(0, 8, size=(rows, K))
    neg = rng.integers(0, 2, size=(rows, K)).astype(bool)
    vals = np.where(neg, -FP4_GRID[mag], FP4_GRID[mag]).astype(np.float32)
    sc = rng.choice(np.asarray(scale_choices, dtype=np.uint8), size=(rows, K // 32))
    ints = np.rint(vals.astype(np.float64) * 2).astype(np.int64) * (1 << (sc.astype(np.int64) - min(scale_choices))).repeat(32, axis=1)
    return export_from_codes(codes_of_values(vals, fmt), sc, fmt), ints


def prove_exact(a_int, w_int):
    """every partial sum of out[m, n] / q (q = 0.25 * both smallest scales) is an integer of magnitude <= sum_k |a_int| |w_int| <=
    max_m sum_k |a_int[m, k]| * max |w_int|, proved in int64: below 2^24 every such integer is an fp32 value, so any summation order gives
    the same bits"""
    bound = int(np.abs(a_int).sum(axis=1).max()) * int(np.abs(w_int).max())
    assert bound < 2 ** 24, f"the test's own inputs are not exactly summable in fp32: bound {bound} >= 2^24"
    return bound
