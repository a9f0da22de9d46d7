"""Independent numpy restatement of the OCP MX fake-quantization rules, on bit patterns.

Shares no code with the product: the shared exponent comes from np.frexp, the element grid from the binade of |t| in float64, and the
export codes from a table of every code's value decoded by the OCP formula (not from the kernel's code arithmetic).

    quantize_bits(bits, dtype, fmt) -> output bit patterns (same shape)
    export_bits(bits, dtype, fmt)   -> (codes uint8 [n_elements] (one per element, unpacked), scales uint8 [n_blocks])
    pack_fp4(codes)                 -> two codes per byte, element 2k in the low nibble of byte k
"""
import numpy as np

BLOCK = 32
# name: (exponent bits, mantissa bits, max normal)
FORMATS = {
    "mxfp4": (2, 1, 6.0),
    "mxfp6_e2m3": (2, 3, 7.5),
    "mxfp6_e3m2": (3, 2, 28.0),
    "mxfp8_e4m3": (4, 3, 448.0),
    "mxfp8_e5m2": (5, 2, 57344.0),
}


def params(fmt):
    """-> (emax_elem, mbits, emin, max normal)"""
    ebits, mbits, maxnorm = FORMATS[fmt]
    bias = 2 ** (ebits - 1) - 1
    return int(np.floor(np.log2(maxnorm))), mbits, 1 - bias, maxnorm


def decode(bits, dtype):
    """bit patterns (uint16 for bf16 / fp16, uint32 for fp32) -> float64 values"""
    bits = np.asarray(bits)
    with np.errstate(invalid="ignore"):   # (signalling NaN patterns widen quietly)
        return _decode(bits, dtype)


def _decode(bits, dtype):
    if dtype == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if dtype == "fp16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def encode(y, dtype):
    """float64 values exact in fp32 (or NaN) -> bit patterns of y rounded once, to nearest-even, to the dtype"""
    f = np.asarray(y, dtype=np.float64).astype(np.float32)   # exact
    if dtype == "fp32":
        return f.view(np.uint32).copy()
    if dtype == "fp16":
        return np.asarray(y, dtype=np.float64).astype(np.float16).view(np.uint16).copy()
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7FC0), r)


def _blocks(bits, dtype):
    v = decode(bits, dtype).reshape(-1, BLOCK)
    finite = np.isfinite(v).all(axis=1)
    vf = np.where(finite[:, None], v, 0.0)
    amax = np.abs(vf).max(axis=1)
    return v, vf, finite, amax


def shared_exp(amax, fmt):
    emax = params(fmt)[0]
    _, e = np.frexp(amax)            # amax = m * 2^e, m in [0.5, 1): floor(log2 amax) = e - 1
    E = np.clip(e.astype(np.int64) - 1 - emax, -127, 127)
    return np.where(amax == 0, -127, E)


def _round_elements(vf, E, fmt):
    """-> q (float64, sign kept) of every element of finite blocks"""
    _, mbits, emin, maxnorm = params(fmt)
    t = vf * np.exp2(-E.astype(np.float64))[:, None]   # exact
    a = np.abs(t)
    _, et = np.frexp(a)
    binade = np.maximum(np.where(a > 0, et.astype(np.int64) - 1, emin), emin)
    quantum = np.exp2((binade - mbits).astype(np.float64))
    qa = np.minimum(np.rint(a / quantum) * quantum, maxnorm)    # np.rint: nearest, ties to even
    return np.copysign(qa, t)


def quantize_values(bits, dtype, fmt):
    """-> y as float64 (exact fp32 values, NaN for non-finite blocks), before the final rounding to the dtype"""
    v, vf, finite, amax = _blocks(bits, dtype)
    E = shared_exp(amax, fmt)
    y = _round_elements(vf, E, fmt) * np.exp2(E.astype(np.float64))[:, None]
    y = np.where(finite[:, None], y, np.nan)
    return y.reshape(np.asarray(bits).shape)


def quantize_bits(bits, dtype, fmt):
    return encode(quantize_values(bits, dtype, fmt), dtype).reshape(np.asarray(bits).shape)


def code_table(fmt):
    """values of the non-negative finite codes 0 .. code(max normal), by the OCP encoding"""
    ebits, mbits, maxnorm = FORMATS[fmt]
    bias = 2 ** (ebits - 1) - 1
    vals = []
    for c in range(2 ** (ebits + mbits)):
        f, m = c >> mbits, c & ((1 << mbits) - 1)
        val = m * 2.0 ** (1 - bias - mbits) if f == 0 else (1 + m / 2 ** mbits) * 2.0 ** (f - bias)
        if val > maxnorm:
            break
        vals.append(val)
    return np.array(vals)


def export_bits(bits, dtype, fmt):
    ebits, mbits, _ = FORMATS[fmt]
    v, vf, finite, amax = _blocks(bits, dtype)
    E = shared_exp(amax, fmt)
    q = _round_elements(vf, E, fmt)
    table = code_table(fmt)
    idx = np.searchsorted(table, np.abs(q))
    assert (table[np.minimum(idx, len(table) - 1)] == np.abs(q)).all(), "q off the element grid"
    codes = idx.astype(np.uint8) | (np.signbit(q).astype(np.uint8) << (ebits + mbits))
    codes = np.where(finite[:, None], codes, 0).astype(np.uint8)
    scales = np.where(finite, E + 127, 0xFF).astype(np.uint8)
    return codes.reshape(-1), scales


def pack_fp4(codes):
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 2)
    return (c[:, 0] | (c[:, 1] << 4)).astype(np.uint8)
