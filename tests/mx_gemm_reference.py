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


# ---- every code of a format, decoded by the OCP formula (not the product's table, not torch's float8 view) ------------------------------
_LAYOUT = {"mxfp4": (2, 1), "mxfp8_e4m3": (4, 3), "mxfp8_e5m2": (5, 2)}   # exponent bits, mantissa bits


def all_code_values(fmt):
    """float64 value of every code 0 .. 2^bits - 1 (sign in the top bit): sub-normal m 2^(1 - bias - mbits), normal (1 + m / 2^mbits)
    2^(f - bias); E4M3 S.1111.111 is NaN, E5M2 S.11111.00 is +-Inf and S.11111.mm NaN; E2M1 has no special code"""
    ebits, mbits = _LAYOUT[fmt]
    bias = 2 ** (ebits - 1) - 1
    vals = np.empty(1 << (1 + ebits + mbits))
    for c in range(vals.size):
        s, f, m = c >> (ebits + mbits), (c >> mbits) & ((1 << ebits) - 1), c & ((1 << mbits) - 1)
        v = m * 2.0 ** (1 - bias - mbits) if f == 0 else (1 + m / 2 ** mbits) * 2.0 ** (f - bias)
        if fmt == "mxfp8_e4m3" and f == 15 and m == 7:
            v = np.nan
        if fmt == "mxfp8_e5m2" and f == 31:
            v = np.inf if m == 0 else np.nan
        vals[c] = -v if s else v
    return vals


def finite_codes(fmt):
    """-> (codes uint8, their values float64, the special codes uint8): every code whose value is finite, both signs and both zeros
    included (16 / 254 / 248 of them), in code order; and the NaN / Inf codes separately"""
    v = all_code_values(fmt)
    fin = np.isfinite(v)
    return np.flatnonzero(fin).astype(np.uint8), v[fin], np.flatnonzero(~fin).astype(np.uint8)


def subnormal_codes(fmt):
    """the nonzero codes of exponent field 0, both signs"""
    ebits, mbits = _LAYOUT[fmt]
    c = np.arange(1 << (1 + ebits + mbits))
    return c[(((c >> mbits) & ((1 << ebits) - 1)) == 0) & ((c & ((1 << mbits) - 1)) != 0)].astype(np.uint8)


def code_of(fmt, value):
    (c,) = np.flatnonzero(all_code_values(fmt) == value)
    return int(c)


def dense(codes, scales, fmt, table=None):
    """codes [rows, K], scales [rows, K / 32] -> float64 [rows, K] = table[code] * 2^(scale - 127), an 0xFF block NaN; table defaults to
    the OCP values.  The decode the seeded-fault test perturbs; test_mx_gemm_cpu.py checks it equal to MXExport.dequantize()."""
    table = all_code_values(fmt) if table is None else table
    s = np.exp2(scales.astype(np.float64) - 127)
    s[scales == 0xFF] = np.nan
    return table[codes] * s.repeat(32, axis=1)


def quantum(values):
    """the largest power of two that every value is an integer multiple of"""
    v = np.abs(np.asarray(values, dtype=np.float64))
    m, e = np.frexp(v[v > 0])
    mant = np.rint(m * 2.0 ** 53).astype(np.int64)            # exact: 53-bit significands
    tz = np.array([(int(x) & -int(x)).bit_length() - 1 for x in mant])
    return 2.0 ** int((e - 53 + tz).min())


def window_codes(rng, rows, K, fmt, codes, scale_choices):
    """-> (codes uint8 [rows, K] drawn from `codes`, scales uint8 [rows, K / 32] drawn from scale_choices, integer form int64 [rows, K]:
    value / quantum(values of `codes`) * 2^(scale - min scale))"""
    codes = np.asarray(list(codes), dtype=np.uint8)
    vals = all_code_values(fmt)[codes]
    assert np.isfinite(vals).all(), "a window holds finite codes only"
    q = quantum(vals)
    pick = rng.integers(0, len(codes), size=(rows, K))
    sc = rng.choice(np.asarray(scale_choices, dtype=np.uint8), size=(rows, K // 32))
    base = vals[pick] / q
    assert np.array_equal(base, np.rint(base))
    ints = base.astype(np.int64) * (1 << (sc.astype(np.int64) - min(scale_choices))).repeat(32, axis=1)
    return codes[pick], sc, ints


def window_operand(rng, rows, K, fmt, codes, scale_choices):
    """grid_operand over an explicit code set -> (CPU MXExport, integer form); window_quantum() is the value of integer 1"""
    c, sc, ints = window_codes(rng, rows, K, fmt, codes, scale_choices)
    return export_from_codes(c, sc, fmt), ints


def window_quantum(fmt, codes, scale_choices):
    return quantum(all_code_values(fmt)[np.asarray(list(codes), dtype=np.uint8)]) * 2.0 ** (min(scale_choices) - 127)


def _both_signs(fmt, lo, hi):
    sign = 1 << sum(_LAYOUT[fmt])
    return list(range(lo, hi + 1)) + [c | sign for c in range(lo, hi + 1)]


# name: (format, codes).  The *_top windows are where ops.mx_export puts every block maximum and most of a Gaussian block; the *_low
# windows hold every sub-normal code and the lowest normal binade.  Integer range after division by the window's quantum in brackets.
WINDOWS = {
    "fp4_full": ("mxfp4", _both_signs("mxfp4", 0, 7)),                    # 0 .. 6        [0 .. 12]
    "e4m3_top": ("mxfp8_e4m3", _both_signs("mxfp8_e4m3", 0x68, 0x7E)),    # 64 .. 448     [8 .. 56]
    "e4m3_top1": ("mxfp8_e4m3", _both_signs("mxfp8_e4m3", 0x78, 0x7E)),   # 256 .. 448    [8 .. 14]
    "e5m2_top": ("mxfp8_e5m2", _both_signs("mxfp8_e5m2", 0x70, 0x7B)),    # 8192 .. 57344 [4 .. 28]
    "e5m2_top1": ("mxfp8_e5m2", _both_signs("mxfp8_e5m2", 0x78, 0x7B)),   # 32768 .. 57344 [4 .. 7]
    "e4m3_low": ("mxfp8_e4m3", _both_signs("mxfp8_e4m3", 0x00, 0x0F)),    # 0 .. 15 * 2^-9 [0 .. 15]
    "e5m2_low": ("mxfp8_e5m2", _both_signs("mxfp8_e5m2", 0x00, 0x07)),    # 0 .. 7 * 2^-16 [0 .. 7]
}
# name: (A window, A scale bytes, W window, W scale bytes).  Each FP8 window meets the full FP4 grid and an FP8 window, in either operand
# position; scale sets of two or three bytes away from 127.  Chosen so that prove_exact passes at every K they are run at (the proof runs
# in the test, on the drawn operands, before anything is launched).
SHORT_K = (128, 384, 1408)
SHORT_SUMS = {
    "e4m3_top x fp4": ("e4m3_top", (126, 127, 128), "fp4_full", (126, 128)),
    "fp4 x e5m2_top": ("fp4_full", (120, 123), "e5m2_top", (127, 128, 129)),
    "e5m2_top x e4m3_top": ("e5m2_top", (127, 129), "e4m3_top", (127, 128)),
    "e4m3_low x e5m2_low": ("e4m3_low", (100, 102, 105), "e5m2_low", (140, 142)),
    "e5m2_low x fp4": ("e5m2_low", (130, 131), "fp4_full", (118, 120, 121)),
    "e4m3_low x e4m3_top": ("e4m3_low", (127, 129), "e4m3_top", (126, 127)),
    "fp4 x e4m3_low": ("fp4_full", (126, 127, 130), "e4m3_low", (90, 91)),
}
LONG_K = (11008, 28672)
LONG_SUMS = {
    "e4m3_top1 x fp4": ("e4m3_top1", (121,), "fp4_full", (126, 127)),
    "fp4 x e4m3_top1": ("fp4_full", (127, 128), "e4m3_top1", (130,)),
    "e4m3_top1 x e5m2_top1": ("e4m3_top1", (125,), "e5m2_top1", (129, 130)),
    "e4m3_low x e5m2_low": ("e4m3_low", (127, 128), "e5m2_low", (100,)),
    "e5m2_top1 x fp4": ("e5m2_top1", (124,), "fp4_full", (126, 128)),
}
SUM_SHAPES = ((13, 100), (29, 203), (150, 203))      # skinny TM = 1, skinny TM = 2, tiled (two tiles in each direction): tails in M and N
LONG_SHAPES = ((13, 52), (29, 52))                   # skinny TM = 1 and 2


def sum_case(family, M, N, K, seed):
    """-> (a_codes, a_scales, a_fmt, w_codes, w_scales, w_fmt, value of integer 1 of the product, a_int, w_int), proved exactly summable"""
    aw, asc, ww, wsc = family
    rng = np.random.default_rng(seed)
    (a_fmt, a_set), (w_fmt, w_set) = WINDOWS[aw], WINDOWS[ww]
    ac, as_, ai = window_codes(rng, M, K, a_fmt, a_set, asc)
    wc, ws_, wi = window_codes(rng, N, K, w_fmt, w_set, wsc)
    prove_exact(ai, wi)
    return ac, as_, a_fmt, wc, ws_, w_fmt, window_quantum(a_fmt, a_set, asc) * window_quantum(w_fmt, w_set, wsc), ai, wi


# ---- single-product operands: the code table and the scale bytes -------------------------------------------------------------------------
TABLE_K = 256


def hot_code_rows(fmt, salt):
    """512 rows: row i carries finite code i + 3 (i // 256) (mod their number) of fmt as its single nonzero, at k = (37 i + salt) mod 256
    -- two walks over every position of two K steps, so that the rows of the zero codes leave no position out --, code 0 elsewhere;
    scales 118 .. 134, different per block and row"""
    fin = finite_codes(fmt)[0]
    i = np.arange(512)
    codes = np.zeros((512, TABLE_K), dtype=np.uint8)
    codes[i, (37 * i + salt) % TABLE_K] = fin[(i + 3 * (i // 256)) % len(fin)]
    r, kb = i[:, None], np.arange(TABLE_K // 32)[None, :]
    return codes, (118 + (r * 7 + kb * 5 + salt) % 17).astype(np.uint8)


def fill_code_rows(fmt, salt):
    """one row per finite code of fmt (repeated up to 48 rows for mxfp4, so that the rows also make a tiled launch), the row filled with
    that code; scales 120 .. 132, different per block and row"""
    fin = finite_codes(fmt)[0]
    rows = max(len(fin), 48)
    codes = np.repeat(fin[np.arange(rows) % len(fin)][:, None], TABLE_K, axis=1)
    r, kb = np.arange(rows)[:, None], np.arange(TABLE_K // 32)[None, :]
    return codes, (120 + (r * 5 + kb * 3 + salt) % 13).astype(np.uint8)


def special_code_rows(fmt):
    """row i: special code i of fmt (NaN, and +-Inf for E5M2) as the single nonzero, k walking over both K steps; all scales 127"""
    sp = finite_codes(fmt)[2]
    codes = np.zeros((len(sp), TABLE_K), dtype=np.uint8)
    i = np.arange(len(sp))
    codes[i, (77 * i + 5) % TABLE_K] = sp
    return codes, np.full((len(sp), TABLE_K // 32), 127, dtype=np.uint8)


def ones_rows(fmt, rows):
    """rows filled with +1.0 (even rows) / -1.0 (odd rows), the last row with zeros; scales 127"""
    one, minus = code_of(fmt, 1.0), code_of(fmt, -1.0)
    codes = np.where(np.arange(rows)[:, None] % 2 == 0, one, minus).astype(np.uint8).repeat(TABLE_K, axis=1)
    codes[-1] = 0
    return codes, np.full((rows, TABLE_K // 32), 127, dtype=np.uint8)


def scale_byte_rows(fmt):
    """1020 rows: row 4 b + g carries scale byte b = 0 .. 254 in block position g = 0 .. 3 of K step b % 2, under a single 1.5 at a k of that
    block; the row's other seven scale bytes are decoys (all different from b, none 0xFF) over zero elements"""
    b, g = np.arange(1020) // 4, np.arange(1020) % 4
    codes = np.zeros((1020, TABLE_K), dtype=np.uint8)
    blk = 4 * (b % 2) + g
    codes[np.arange(1020), 32 * blk + (7 * (b // 2) + 3 * g) % 32] = code_of(fmt, 1.5)     # every k of both steps is some row's
    kb = np.arange(TABLE_K // 32)[None, :]
    scales = (b[:, None] + 1 + 31 * (kb + 1)) % 255
    scales[np.arange(1020), blk] = b
    return codes, scales.astype(np.uint8)


def scale_partner_rows(fmt):
    """255 rows of nonzero normal codes that differ along k and rows; row n's scale bytes lie within 2 of 254 - n, so that against scale byte
    b the product's exponent is about b - n: normal in fp32 for |b - n| below about 100, beyond the sub-normal range / above the maximum at
    the far ends"""
    r, k = np.arange(255)[:, None], np.arange(TABLE_K)[None, :]
    if fmt == "mxfp4":
        codes = (r * 3 + k * 5) % 7 + 1 + 8 * ((r + k // 3) % 2)
    else:
        codes = (r * 37 + k * 11) % 100 + 8 + 128 * ((r + k // 3) % 2)
    kb = np.arange(TABLE_K // 32)[None, :]
    top = 254 - {"mxfp4": 3, "mxfp8_e4m3": 7, "mxfp8_e5m2": 12}[fmt]       # |element| < 2^3 / 2^7 / 2^12: element * scale stays an fp32 value,
    scales = np.clip(254 - r + (kb * 3 + r) % 5 - 2, 0, top)               # so that dequantize() in float32 is exact
    return codes.astype(np.uint8), scales.astype(np.uint8)


F32_TINY, F32_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)


def normal_or_zero(ref):
    """ref: float64 tensor -> mask of the results that are zero or normal fp32 values (no rounding can happen on the way to fp32 for a
    single product of two at most 4-bit significands)"""
    a = ref.abs()
    return (a == 0) | ((a >= F32_TINY) & (a <= F32_MAX))
