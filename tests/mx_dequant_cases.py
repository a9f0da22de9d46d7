"""Case sets of the MX dequantize tests, shared by the CPU tier (tests/test_mx_dequant_cpu.py, which shows the
exhaustive set to be sensitive to a wrong scale and a wrong element table on the reference alone) and the GPU tier
(tests/test_gpu_mx_dequant.py, which runs the kernel on it).  The reference is ops.MXExport.dequantize() on CPU tensors throughout."""
import numpy as np
import torch

from llm_qat_amd import ops

FMTS = ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2")
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
IDT = {"bf16": torch.int16, "fp16": torch.int16, "fp32": torch.int32}
NDT = {"bf16": np.uint16, "fp16": np.uint16, "fp32": np.uint32}
DTYPES = tuple(TDT)


def exhaustive(fmt):
    """Every code under every scale byte -> (elements, scales, shape), CPU uint8 tensors: 256 rows, row s carries scale byte s in all its
    blocks.  mxfp4: shape [256, 32], one block per row whose byte k is code k in the low nibble and code 15 - k in the high one (every
    code in both nibbles); mxfp8_*: shape [256, 256], column c holds code c."""
    s = torch.arange(256, dtype=torch.uint8)
    if fmt == "mxfp4":
        k = torch.arange(16, dtype=torch.uint8)
        return (k | ((15 - k) << 4)).repeat(256, 1), s.reshape(256, 1).clone(), (256, 32)
    return s.repeat(256, 1), s.reshape(256, 1).repeat(1, 8), (256, 256)


def codes_of(fmt):
    """the code of every element of exhaustive(fmt)'s rows, [cols] ints"""
    if fmt == "mxfp4":
        k = np.arange(16)
        return np.stack((k, 15 - k), -1).reshape(-1)
    return np.arange(256)


def finite_nonzero(fmt):
    """mask over the codes 0 .. 15 / 0 .. 255: finite and not a zero"""
    c = np.arange(16 if fmt == "mxfp4" else 256)
    if fmt == "mxfp4":
        return (c & 7) != 0
    mag = c & 0x7F
    return (mag != 0) & ((mag != 0x7F) if fmt == "mxfp8_e4m3" else (mag < 0x7C))


def next_code(fmt):
    """a wrong element table: every finite non-zero code -> the code one mantissa step up, same sign (the largest one wraps to the
    smallest); the other codes stay.  [16] / [256] uint8"""
    n = 16 if fmt == "mxfp4" else 256
    signbit = n // 2
    ok = finite_nonzero(fmt)
    mags = [m for m in range(signbit) if ok[m]]
    nxt = {m: mags[(i + 1) % len(mags)] for i, m in enumerate(mags)}
    return np.array([(c & signbit) | nxt[c & (signbit - 1)] if ok[c] else c for c in range(n)], dtype=np.uint8)


def remap(elements, fmt, table):
    """elements with every code sent through table ([16] / [256] uint8)"""
    e = elements.numpy()
    t = np.asarray(table, dtype=np.uint8)
    out = (t[e & 0xF] | (t[e >> 4] << 4)) if fmt == "mxfp4" else t[e]
    return torch.from_numpy(out.astype(np.uint8))


def reference(elements, scales, fmt, shape, dtype):
    """ops.MXExport.dequantize() on CPU copies -> a CPU tensor of `shape` in TDT[dtype]"""
    return ops.MXExport(elements.cpu(), scales.cpu(), fmt, tuple(shape), TDT[dtype]).dequantize()


def bits(t, dtype):
    return t.detach().contiguous().cpu().view(IDT[dtype]).numpy().view(NDT[dtype])


def random_export(nblocks, fmt, seed):
    """nblocks blocks of random code bytes (every byte value: the FP8 NaN / Inf codes included) under random scale bytes, 0 and 0xFF among
    them -> (elements, scales, shape [nblocks, 32]), CPU uint8"""
    g = torch.Generator().manual_seed(seed)
    elements = torch.randint(0, 256, (nblocks, 16 if fmt == "mxfp4" else 32), generator=g, dtype=torch.uint8)
    scales = torch.randint(0, 256, (nblocks, 1), generator=g, dtype=torch.uint8)
    scales[0, 0], scales[-1, 0] = 0, 0xFF
    return elements, scales, (nblocks, 32)
