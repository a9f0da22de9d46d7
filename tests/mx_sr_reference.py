"""numpy restatement of MX fake quantization with stochastic rounding, on bit patterns.  Shares no code with the
product: its own Philox4x32-10 in uint64 arithmetic, the rounding rule restated on the float64 grid logic of mx_reference /
mx_rules_reference (whose decode / encode, shared exponents and format table it uses).

    philox4x32_10(counter [n, 4], key (k0, k1))           -> uint32 [n, 4]
    r16(seed, stream, idx)                                -> the 16-bit random number of flat elements idx (any integer array)
    quantize_bits(bits, dtype, fmt, rule, seed, stream, axis=-1)   -> output bit patterns, the shape of bits
    parts(bits, dtype, fmt, rule, seed, stream, axis=-1)  -> dict of float64 arrays, the shape of bits: x (the input), lo / hi (the two
                                                             grid neighbours of |x| times the block's scale, saturation applied), y (the
                                                             output before the rounding to the dtype), finite (bool)

The flat index of an element is its row-major position in the contiguous tensor; axis=-2 runs the blocks down the second-to-last
dimension and leaves the indices as they are.  The rule, per element of a finite block with shared exponent E (floor or ceil rule):
    t = fp32(v * 2^-E);  a = |t| / quantum (quantum of t's binade, clamped at the smallest normal one);  n = floor(a), f = a - n
    up = R16 < f * 65536;  q = min((n + up) * quantum, max-normal) with v's sign;  y = q * 2^E, rounded once to the dtype
"""
import numpy as np

from mx_reference import BLOCK, decode, encode, params
from mx_rules_reference import shared_exp

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    c = np.asarray(counter, dtype=np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & LOW, n2, p0 & LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def r16(seed, stream, idx):
    """R16 of the flat elements idx: word[(i & 7) >> 1] of the call with counter (i >> 3, stream), its low half for even i"""
    idx = np.asarray(idx, dtype=np.uint64)
    flat = idx.reshape(-1)
    cnt, inv = np.unique(flat >> np.uint64(3), return_inverse=True)
    ctr = np.stack([cnt & LOW, cnt >> S32, np.full_like(cnt, int(stream) & 0xFFFFFFFF), np.full_like(cnt, int(stream) >> 32)], axis=1)
    words = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    j = (flat & np.uint64(7)).astype(np.int64)
    w = words[inv.reshape(-1), j >> 1]
    return ((w >> (16 * (j & 1)).astype(np.uint32)) & np.uint32(0xFFFF)).astype(np.uint16).reshape(idx.shape)


def _to_blocks(arr, axis):
    """arr with the block axis last, as [n_blocks, 32]; -> (blocks, undo)"""
    a = np.asarray(arr)
    if axis == -2:
        a = np.swapaxes(a, -1, -2)
    shape = a.shape
    return np.ascontiguousarray(a).reshape(-1, BLOCK), (lambda b: np.ascontiguousarray(np.swapaxes(b.reshape(shape), -1, -2)) if axis == -2 else b.reshape(shape))


def parts(bits, dtype, fmt, rule, seed, stream, axis=-1, first=0):
    """first: the flat index of the tensor's first element (a slice of a larger launch)"""
    assert axis in (-1, -2)
    bits = np.asarray(bits)
    _, mbits, emin, maxnorm = params(fmt)
    v, undo = _to_blocks(decode(bits, dtype), axis)
    idx, _ = _to_blocks(np.arange(bits.size, dtype=np.uint64).reshape(bits.shape) + np.uint64(first), axis)
    finite = np.isfinite(v).all(axis=1)
    vf = np.where(finite[:, None], v, 0.0)
    E = shared_exp(np.abs(vf).max(axis=1), fmt, rule).astype(np.float64)[:, None]
    with np.errstate(under="ignore"):
        t = (vf * np.exp2(-E)).astype(np.float32).astype(np.float64)          # the product is an fp32 value: it may underflow far below the grid
    a = np.abs(t)
    _, et = np.frexp(a)
    binade = np.maximum(np.where(a > 0, et.astype(np.int64) - 1, emin), emin)
    quantum = np.exp2((binade - mbits).astype(np.float64))
    aq = a / quantum                                                          # exact: a power-of-two scaling
    n = np.floor(aq)
    f = aq - n
    up = r16(seed, stream, idx).astype(np.float64) < f * 65536.0
    scale = np.exp2(E)
    lo = np.minimum(n * quantum, maxnorm) * scale
    hi = np.minimum((n + 1) * quantum, maxnorm) * scale
    y = np.copysign(np.where(up, hi, lo), vf)
    fin = np.broadcast_to(finite[:, None], v.shape)
    return {"x": undo(v), "lo": undo(lo), "hi": undo(hi), "y": undo(np.where(fin, y, np.nan)), "finite": undo(fin), "up": undo(up & fin)}


def quantize_bits(bits, dtype, fmt, rule, seed, stream, axis=-1, first=0):
    with np.errstate(over="ignore"):   # a block near the top of fp32 may round up to Inf in the one rounding to the dtype
        return encode(parts(bits, dtype, fmt, rule, seed, stream, axis, first)["y"], dtype).reshape(np.asarray(bits).shape)
