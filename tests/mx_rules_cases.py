"""Inputs of the scale-rule / saturation-mask tests, shared by the CPU tier (which proves them sensitive against deliberately wrong
references) and the GPU tier (which runs the kernels on them).  numpy only."""
import numpy as np

from mx_reference import decode, encode, params

FMTS = ["mxfp4", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e4m3", "mxfp8_e5m2"]
EXPORT_FMTS = ["mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"]
# the amax list of tests/test_gpu_mx.py::exhaustive_bits
LEADS = [1.0, 5.0, 7.5, 2.0 ** -126, 2.0 ** -133, 3e38, 0.1, 448.0, 1000.0, 65504.0, 6e-8]


def lead_bits(dtype, fmt):
    """16-bit patterns of the block leaders: LEADS rounded to the dtype (finite, non-zero), the dtype's largest finite value, and the
    format's max-normal mantissa exactly, one ulp below and one ulp above, at the format's own binade and ten binades below"""
    out = []
    for a in LEADS:
        b = int(encode(np.array([a]), dtype)[0])
        v = decode(np.array([b], np.uint16), dtype)[0]
        if np.isfinite(v) and v != 0:
            out.append(b)
    out.append({"bf16": 0x7F7F, "fp16": 0x7BFF}[dtype])      # the dtype's largest finite value: every finite pattern is below some leader
    maxnorm = params(fmt)[3]
    for scale in (1.0, 2.0 ** -10):
        b = int(encode(np.array([maxnorm * scale]), dtype)[0])
        assert decode(np.array([b], np.uint16), dtype)[0] == maxnorm * scale
        out += [b - 1, b, b + 1]
    return out


def exhaustive_bits(dtype, fmt):
    """every 16-bit pattern, arranged as tests/test_gpu_mx.py does: the finite ones in blocks led by a chosen amax (each block holds only
    patterns with |v| <= that amax), the non-finite ones in blocks of their own -> uint16 [n, 256]"""
    allb = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    v = decode(allb, dtype)
    fin = np.isfinite(v)
    blocks = []
    for lb in lead_bits(dtype, fmt):
        a = abs(decode(np.array([lb], np.uint16), dtype)[0])
        cand = allb[fin & (np.abs(v) <= a)]
        cand = np.concatenate([cand, np.zeros((-len(cand)) % 31, np.uint16)]).reshape(-1, 31)
        blocks.append(np.concatenate([np.full((len(cand), 1), lb, np.uint16), cand], 1))
    nonfin = allb[~fin]
    blocks.append(np.concatenate([nonfin, np.full((-len(nonfin)) % 32, 0x3F80 if dtype == "bf16" else 0x3C00, np.uint16)]).reshape(-1, 32))
    out = np.concatenate(blocks, 0).reshape(-1)
    return np.concatenate([out, np.zeros((-out.size) % 256, np.uint16)]).reshape(-1, 256)


def rand_bits(shape, dtype, seed):
    """values over many binades, with zeros, signed zeros, tiny values and a few non-finite elements -> bit patterns of `shape`"""
    rng = np.random.default_rng(seed)
    nb = int(np.prod(shape)) // 32
    x = rng.standard_normal((nb, 32)) * np.exp2(rng.integers(-30, 30, (nb, 1)).astype(np.float64))
    x = x.astype(np.float32).astype(np.float64).reshape(-1)
    n = x.size
    idx = rng.integers(0, n, max(3, n // 1000))
    k = len(idx) // 3
    x[idx[:k]] = -0.0
    x[idx[k:2 * k]] = 1e-41
    b = encode(x, dtype).reshape(-1).copy()
    nan = {"bf16": 0x7FC1, "fp16": 0x7E01, "fp32": 0x7FC00001}[dtype]
    inf = {"bf16": 0xFF80, "fp16": 0xFC00, "fp32": 0xFF800000}[dtype]
    b[idx[-2:]] = nan
    b[idx[-3]] = inf
    return b.reshape(shape)


def grad_bits(keep, dtype, seed):
    """a gradient of keep's shape whose NaN, +Inf, -Inf and -0.0 sit at masked and at kept positions alike"""
    keep = np.asarray(keep, dtype=bool)
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(keep.size).astype(np.float32).astype(np.float64)
    b = encode(g, dtype).reshape(-1).copy()
    special = {"bf16": (0x7FC0, 0x7F80, 0xFF80, 0x8000, 0x7FFF), "fp16": (0x7E00, 0x7C00, 0xFC00, 0x8000, 0x7FFF),
               "fp32": (0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x7FFFFFFF)}[dtype]
    flat = keep.reshape(-1)
    for sel in (np.flatnonzero(~flat), np.flatnonzero(flat)):
        if sel.size:
            pick = sel[rng.integers(0, sel.size, min(sel.size, 40))]
            for j, p in enumerate(pick):
                b[p] = special[j % len(special)]
    return b.reshape(keep.shape)
