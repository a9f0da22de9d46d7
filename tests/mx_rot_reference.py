"""numpy restatement of the 64-wide block-Hadamard rotation that the rotated MX entry points apply before they quantize (DESIGN.md section
15).  It shares no code with the product and composes with mx_reference: the rotated fp32 values go through quantize_values / export_bits
as "fp32" input and are rounded once to the tensor's dtype by encode.

Definition, per run of 64 consecutive elements of the last dimension: widen to fp32; for s = 1, 2, 4, 8, 16, 32 in that order, for every
element index j of the run with bit s clear, (v[j], v[j+s]) <- (v[j] + v[j+s], v[j] - v[j+s]), every add / subtract one IEEE fp32
operation; then multiply by 0.125f."""
import numpy as np

from mx_reference import decode, encode, export_bits, quantize_values

RUN = 64


def hadamard64():
    """H64 as float64: entry (i, j) = (-1)^popcount(i & j)"""
    i = np.arange(RUN)
    return np.array([[(-1.0) ** bin(a & b).count("1") for b in i] for a in i], dtype=np.float64)


def rotate_f32(v):
    """float32 array [..., 64 k] -> its rotation, float32 (numpy adds and subtracts float32 arrays in float32, one rounding each)"""
    v = np.asarray(v)
    assert v.dtype == np.float32 and v.shape[-1] % RUN == 0
    r = v.reshape(-1, RUN).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for s in (1, 2, 4, 8, 16, 32):
            # element index j = (c * 2 + h) * s + i: h is bit s of j, so [:, :, 0, :] are the j with the bit clear and [:, :, 1, :] their j + s
            p = r.reshape(-1, RUN // (2 * s), 2, s)
            a, b = p[:, :, 0, :].copy(), p[:, :, 1, :].copy()
            p[:, :, 0, :] = a + b
            p[:, :, 1, :] = a - b
        r = r * np.float32(0.125)
    assert r.dtype == np.float32
    return r.reshape(v.shape)


def rotate_values(bits, dtype):
    """bit patterns of a [..., 64 k] tensor of `dtype` -> the fp32 values of x R"""
    with np.errstate(invalid="ignore"):
        return rotate_f32(decode(bits, dtype).astype(np.float32))    # (every bf16 / fp16 / fp32 value is exact in float32)


def rotate_bits(bits, dtype):
    """fq_block_rotate: the rotated fp32 values rounded once to the dtype"""
    return encode(rotate_values(bits, dtype).astype(np.float64), dtype).reshape(np.asarray(bits).shape)


def quantize_rot_bits(bits, dtype, fmt):
    """fq_mx_fwd_rot: MX quantization of the rotated fp32 values, rounded once to the dtype"""
    r = rotate_values(bits, dtype)
    return encode(quantize_values(r.view(np.uint32), "fp32", fmt), dtype).reshape(np.asarray(bits).shape)


def export_rot_bits(bits, dtype, fmt):
    """fq_mx_export_rot -> (codes, scales) of the rotated fp32 values"""
    return export_bits(rotate_values(bits, dtype).view(np.uint32), "fp32", fmt)
