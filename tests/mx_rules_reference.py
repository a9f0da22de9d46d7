"""numpy restatement of the MX scale rules, the saturation mask and the masked straight-through backward, on bit
patterns.  Shares no code with the product.  The shared exponent is read from the fp32 bits of amax by integer arithmetic (not np.frexp, as
mx_reference does, so the two floor rules check each other), the element rounding is restated here so that the value on the UNBOUNDED grid
is at hand, and the bit patterns go in and out through mx_reference's decode / encode and mx_rot_reference's rotation.

    shared_exp(amax, fmt, rule)               -> E per block ("floor" / "ceil")
    quantize_bits(bits, dtype, fmt, rule)     -> output bit patterns            (rotate=True: of the fp32 values of x R)
    export_bits(bits, dtype, fmt, rule)       -> (codes uint8 [n], scales uint8 [n / 32])
    keep_mask(bits, dtype, fmt, rule)         -> bool per element: False iff saturation changed the rounded value
    pack_mask(keep)                           -> uint8 [n / 8]: bit i & 7 of byte i >> 3 is element i
    ste_backward_bits(gbits, keep, dtype, rotate) -> bit patterns of g where keep, +0.0 elsewhere (rotate: times R, rounded once)
"""
import numpy as np

from mx_reference import BLOCK, code_table, decode, encode, params, FORMATS
from mx_rot_reference import rotate_bits, rotate_values

RULES = ("floor", "ceil")


def _amax_exponent(amax):
    """floor(log2 amax) of positive float64 values that are exact in fp32, from the fp32 bits (subnormals by the top set bit)"""
    u = np.asarray(amax, dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.int64)
    f = (u >> 23) & 0xFF
    man = u & 0x7FFFFF
    top = np.zeros_like(man)
    for b in range(23):                     # position of the highest set mantissa bit (subnormal amax)
        top = np.where((man >> b) & 1 == 1, b, top)
    return np.where(f > 0, f - 127, top - 149)


def shared_exp(amax, fmt, rule="floor"):
    assert rule in RULES
    emax, _, _, maxnorm = params(fmt)
    amax = np.asarray(amax, dtype=np.float64)
    safe = np.where(amax > 0, amax, 1.0)
    Ef = _amax_exponent(safe) - emax        # unclamped
    if rule == "ceil":
        t = safe * np.exp2(-Ef.astype(np.float64))      # exact: in [2^emax, 2^(emax + 1))
        Ef = np.where(t > maxnorm, Ef + 1, Ef)
    E = np.clip(Ef, -127, 127)
    return np.where(amax == 0, -127, E)


def _blocks(bits, dtype):
    v = decode(bits, dtype).reshape(-1, BLOCK)
    finite = np.isfinite(v).all(axis=1)
    vf = np.where(finite[:, None], v, 0.0)
    return vf, finite, np.abs(vf).max(axis=1)


def round_unbounded(vf, E, fmt):
    """-> (|t| rounded to nearest-even onto the element grid extended upwards without bound, t) for finite blocks"""
    _, mbits, emin, _ = params(fmt)
    t = vf * np.exp2(-E.astype(np.float64))[:, None]
    a = np.abs(t)
    with np.errstate(divide="ignore"):
        binade = np.where(a > 0, np.floor(np.log2(np.where(a > 0, a, 1.0))), emin)
    # log2 of a float64 just below a power of two may round up to it: put such values back into their binade
    binade = np.where(np.exp2(binade) > np.where(a > 0, a, np.inf), binade - 1, binade)
    binade = np.maximum(binade, emin)
    quantum = np.exp2(binade - mbits)
    return np.rint(a / quantum) * quantum, t


def _source_bits(bits, dtype, rotate):
    """the tensor the quantizer sees: the bits themselves, or the fp32 values of x R"""
    if rotate:
        return rotate_values(bits, dtype).view(np.uint32), "fp32"
    return np.asarray(bits), dtype


def _quantize(bits, dtype, fmt, rule, rotate):
    src, sdt = _source_bits(bits, dtype, rotate)
    vf, finite, amax = _blocks(src, sdt)
    E = shared_exp(amax, fmt, rule)
    maxnorm = params(fmt)[3]
    ru, t = round_unbounded(vf, E, fmt)
    q = np.copysign(np.minimum(ru, maxnorm), t)
    keep = ~(ru > maxnorm) | ~finite[:, None]
    return q, E, finite, keep


def quantize_values(bits, dtype, fmt, rule="floor", rotate=False):
    q, E, finite, _ = _quantize(bits, dtype, fmt, rule, rotate)
    y = q * np.exp2(E.astype(np.float64))[:, None]
    return np.where(finite[:, None], y, np.nan).reshape(np.asarray(bits).shape)


def quantize_bits(bits, dtype, fmt, rule="floor", rotate=False):
    with np.errstate(over="ignore"):   # a block near the top of fp32 may round up to Inf in the one rounding to the dtype
        return encode(quantize_values(bits, dtype, fmt, rule, rotate), dtype).reshape(np.asarray(bits).shape)


def export_bits(bits, dtype, fmt, rule="floor", rotate=False):
    ebits, mbits, _ = FORMATS[fmt]
    q, E, finite, _ = _quantize(bits, dtype, fmt, rule, rotate)
    table = code_table(fmt)
    idx = np.searchsorted(table, np.abs(q))
    assert (table[np.minimum(idx, len(table) - 1)] == np.abs(q)).all(), "q off the element grid"
    codes = idx.astype(np.uint8) | (np.signbit(q).astype(np.uint8) << (ebits + mbits))
    codes = np.where(finite[:, None], codes, 0).astype(np.uint8)
    return codes.reshape(-1), np.where(finite, E + 127, 0xFF).astype(np.uint8)


def keep_mask(bits, dtype, fmt, rule="floor", rotate=False):
    """bool, the shape of bits: False iff the value rounded on the unbounded grid exceeds max-normal in magnitude (NaN / Inf blocks and
    amax == 0 blocks: all True)"""
    return _quantize(bits, dtype, fmt, rule, rotate)[3].reshape(np.asarray(bits).shape)


def pack_mask(keep):
    return np.packbits(np.asarray(keep, dtype=bool).reshape(-1), bitorder="little")


def unpack_mask(mask_bytes, n):
    return np.unpackbits(np.asarray(mask_bytes, dtype=np.uint8).reshape(-1), bitorder="little")[:n].astype(bool)


def ste_backward_bits(gbits, keep, dtype, rotate=False):
    gbits = np.asarray(gbits)
    masked = np.where(np.asarray(keep, dtype=bool).reshape(gbits.shape), gbits, gbits.dtype.type(0))
    with np.errstate(over="ignore", invalid="ignore"):
        return rotate_bits(masked, dtype) if rotate else masked
