"""MX block-scaled GEMM, CPU tier (no GPU): argument errors of ops.mx_matmul, every fq_mx_gemm validation code (validation comes before
any launch), the header / EXPORTS agreement, MXLinear eligibility and its state_dict, and the float64 reference on worked values."""
import os
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import MXLinear, _lib, convert_to_mx_inference, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_gemm_reference import codes_of_values, export_from_codes, grid_operand, prove_exact, ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _export(rows, K, fmt="mxfp4"):
    return export_from_codes(np.zeros((rows, K), np.uint8), np.full((rows, K // 32), 127, np.uint8), fmt)


def test_mx_matmul_argument_errors():
    a, w = _export(4, 256), _export(8, 256)
    with pytest.raises(TypeError):
        ops.mx_matmul(a.elements, w)
    with pytest.raises(ValueError, match="K=256 but w has K=128"):
        ops.mx_matmul(a, _export(8, 128))
    with pytest.raises(ValueError, match="not served"):
        ops.mx_matmul(_export(4, 96), _export(8, 96))           # a multiple of 32, not of the kernel's 128
    with pytest.raises(ValueError, match="2-D"):
        ops.mx_matmul(a, ops.MXExport(w.elements, w.scales, "mxfp4", (2, 4, 256), torch.float32))
    for bad in ("mxfp6_e2m3", "mxfp6_e3m2"):
        with pytest.raises(ValueError, match="FP6"):
            ops.mx_matmul(ops.MXExport(a.elements, a.scales, bad, a.shape, a.dtype), w)
        with pytest.raises(ValueError, match="FP6"):
            ops.mx_matmul(a, ops.MXExport(w.elements, w.scales, bad, w.shape, w.dtype))
    with pytest.raises(ValueError, match="unknown MX format"):
        ops.mx_matmul(ops.MXExport(a.elements, a.scales, "int4", a.shape, a.dtype), w)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.mx_matmul(a, w, out_dtype=torch.float64)
    for allow in (False, True):                                  # CPU tensors raise like the rest of the MX path
        llm_qat_amd.allow_cpu_tensors(allow)
        try:
            with pytest.raises(RuntimeError, match="no CPU"):
                ops.mx_matmul(a, w)
        finally:
            llm_qat_amd.allow_cpu_tensors(False)
    assert "mx_gemm_launch" not in llm_qat_amd.stats()


def test_fq_mx_gemm_validation_codes():
    L = _lib.lib()
    f = 1 << 20       # 16-byte-aligned non-NULL addresses: never dereferenced, validation fails first
    ok = dict(a_fmt=3, w_fmt=0, M=4, N=8, K=256, dt=_lib.DTYPE_BF16, ae=f, asc=f + 4096, we=f + 8192, wsc=f + 12288, out=f + 16384)

    def call(**kw):
        p = dict(ok, **kw)
        return L.fq_mx_gemm(p["ae"], p["asc"], p["a_fmt"], p["we"], p["wsc"], p["w_fmt"], p["out"], p["M"], p["N"], p["K"], p["dt"], None)

    assert call(dt=_lib.DTYPE_F64) == -1 and call(dt=9) == -1 and call(dt=-1) == -1
    for fmt in (1, 2, 5, -1):                                   # FP6 and unknown codes, either operand
        assert call(a_fmt=fmt) == -7 and call(w_fmt=fmt) == -7
    assert call(M=-1) == -3 and call(N=-1) == -3 and call(K=-128) == -3
    assert call(K=96) == -3 and call(K=32) == -3 and call(K=0) == -3          # K: a positive multiple of 128
    assert call(M=2 ** 31) == -3 and call(N=2 ** 40) == -3 and call(K=2 ** 31) == -3
    for p in ("ae", "asc", "we", "wsc", "out"):
        assert call(**{p: None}) == -4
    for p in ("ae", "we", "out"):
        assert call(**{p: f + 8}) == -8
    assert call(M=33, N=128 * 65535 + 1) == -8                                 # beyond one launch's grid
    assert call(M=0, ae=None, asc=None, out=None) == 0 and call(N=0, we=None, wsc=None, out=None) == 0   # empty: no launch
    assert b"" == L.fq_last_error()


def test_header_declares_fq_mx_gemm_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "llmqat_fakequant.h")).read()
    m = re.search(r"^int fq_mx_gemm\(([^;]*)\);", hdr, re.M | re.S)
    assert m, "fq_mx_gemm is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = ["p" if "*" in p else "q" if p.startswith("int64_t") else "i" for p in params]
    assert "".join(kinds) == "ppippipqqqip"                      # pointers, int, int64 and the stream only
    assert "fq_mx_gemm" in _lib.EXPORTS
    L = _lib.lib()
    import ctypes
    assert [("p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64 else "i") for t in L.fq_mx_gemm.argtypes] == kinds
    assert L.fq_version() == _lib.ABI_VERSION


def test_abi_fuzz_and_export_tests_pass_with_the_new_name():
    import test_abi_and_host as T
    T.test_library_exports_every_declared_symbol()
    T.test_abi_rejects_null_pointers_and_hostile_sizes_before_any_launch()


def test_mx_linear_eligibility_errors():
    F = MXLinear.from_quantize_linear
    with pytest.raises(ValueError, match="expected a QuantizeLinear"):
        F(torch.nn.Linear(256, 64))
    with pytest.raises(ValueError, match="weight_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8))                                           # integer-quantized
    with pytest.raises(ValueError, match="act_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_format="mxfp4"))
    with pytest.raises(ValueError, match="weight_format is not set"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_group_size=32, act_format="mxfp8_e4m3"))   # group-wise weight
    with pytest.raises(ValueError, match="no export packing"):
        F(QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_format="mxfp6_e2m3", act_format="mxfp8_e4m3"))
    with pytest.raises(ValueError, match="in_features=96"):
        F(QuantizeLinear(96, 64, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3"))
    with pytest.raises(ValueError):
        MXLinear(96, 64)
    with pytest.raises(ValueError):
        MXLinear(256, 64, weight_format="mxfp6_e3m2")
    prev = llm_qat_amd.default_mx_formats("mxfp4", "mxfp8_e4m3")   # formats through the process default resolve too: only the device is missing
    try:
        layer = QuantizeLinear(256, 64, w_bits=4, a_bits=8)
    finally:
        llm_qat_amd.default_mx_formats(*prev)
    with pytest.raises(RuntimeError, match="no CPU"):
        F(layer)
    model = torch.nn.Sequential(QuantizeLinear(256, 64, w_bits=8, a_bits=8), torch.nn.Linear(64, 8),
                                QuantizeLinear(96, 64, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3"))
    kept = list(model)
    assert convert_to_mx_inference(model) == 0 and all(a is b for a, b in zip(model, kept))


def test_mx_linear_state_dict_round_trip_and_no_float_weight():
    torch.manual_seed(0)
    m = MXLinear(256, 64, "mxfp4", "mxfp8_e4m3", bias=True, dtype=torch.bfloat16)
    assert m.weight_elements.shape == (64, 128) and m.weight_scales.shape == (64, 8) and m.bias.shape == (64,)
    assert MXLinear(256, 64, "mxfp8_e5m2", "mxfp4").weight_elements.shape == (64, 256)
    assert list(m.parameters()) == [] and sorted(m.state_dict()) == ["bias", "weight_elements", "weight_scales"]
    m.weight_elements.copy_(torch.randint(0, 256, (64, 128), dtype=torch.uint8))
    m.weight_scales.copy_(torch.randint(100, 140, (64, 8), dtype=torch.uint8))
    m.bias.normal_()
    m2 = MXLinear(256, 64, "mxfp4", "mxfp8_e4m3", bias=True, dtype=torch.bfloat16)
    m2.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]) and v.dtype == m2.state_dict()[k].dtype
    assert sorted(MXLinear(256, 64).state_dict()) == ["weight_elements", "weight_scales"]
    with pytest.raises(RuntimeError):                                # a layer of another shape does not load
        MXLinear(512, 64).load_state_dict(m.state_dict())
    x = torch.zeros(2, 256, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m(x)


def test_reference_on_worked_values():
    """A row [1.5, -2, 0...] x 2^1 (block 0) and [6, 0.5, 0...] x 2^-2 (block 4), W rows with the matching elements: by hand."""
    K = 256
    av = np.zeros((1, K), np.float32)
    av[0, 0], av[0, 1], av[0, 128], av[0, 129] = 1.5, -2.0, 6.0, 0.5
    asc = np.full((1, K // 32), 127, np.uint8)
    asc[0, 0], asc[0, 4] = 128, 125
    wv = np.zeros((2, K), np.float32)
    wv[0, 0], wv[0, 1], wv[0, 128] = 4.0, 3.0, -1.0
    wv[1, 129], wv[1, 2] = -6.0, 6.0
    wsc = np.full((2, K // 32), 127, np.uint8)
    wsc[0, 0], wsc[0, 4], wsc[1, 4] = 126, 130, 0x7E
    for a_fmt in ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"):
        for w_fmt in ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"):
            a = export_from_codes(codes_of_values(av, a_fmt), asc, a_fmt)
            w = export_from_codes(codes_of_values(wv, w_fmt), wsc, w_fmt)
            ref, S = ref64(a, w)
            # out[0, 0] = (3 * 2 + -4 * 1.5) [block 0: A x2, W x0.5] + (1.5 * -8) [block 4: 6 x 2^-2 times -1 x 2^3] = 0 - 12
            # out[0, 1] = 0.5 * 2^-2 * -6 * 2^-1 = -0.375
            assert ref.tolist() == [[-12.0, -0.375]]
            assert S.tolist() == [[3 * 2 + 4 * 1.5 + 12.0, 0.375]]
    a.scales[0, 7] = 0xFF                                            # an 0xFF block anywhere in the row poisons the row
    assert torch.isnan(ref64(a, w)[0]).all()
    z = export_from_codes(np.full((1, K), 2, np.uint8), np.zeros((1, K // 32), np.uint8), "mxfp4")     # scale byte 0 is 2^-127
    big = export_from_codes(np.full((1, K), 2, np.uint8), np.full((1, K // 32), 254, np.uint8), "mxfp4")
    assert ref64(z, big)[0].item() == 256.0


def test_exactness_proof_rejects_inputs_that_could_round():
    rng = np.random.default_rng(0)
    a, ai = grid_operand(rng, 4, 4096, "mxfp4")
    w, wi = grid_operand(rng, 8, 4096, "mxfp8_e4m3")
    assert prove_exact(ai, wi) < 2 ** 24
    ref, _ = ref64(a, w)
    assert torch.equal(ref, torch.from_numpy((ai @ wi.T).astype(np.float64) * 0.25))
    with pytest.raises(AssertionError):
        prove_exact(ai * 64, wi)


def test_the_product_does_not_import_tools_or_oracle():
    src = open(os.path.join(ROOT, "llm-qat_amd", "mx_inference.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(tools|oracle)\b", src, re.M)


# ---- the helpers and the families of tests/test_gpu_mx_gemm_codes.py: proved, and proved sensitive, without a GPU ----------------------
import mx_gemm_reference as R
from mx_reference import code_table, export_bits


def test_finite_codes_by_the_ocp_formula_agree_with_torch_float8():
    for fmt, n, special in (("mxfp4", 16, []), ("mxfp8_e4m3", 254, [0x7F, 0xFF]), ("mxfp8_e5m2", 248, [0x7C, 0x7D, 0x7E, 0x7F, 0xFC, 0xFD, 0xFE, 0xFF])):
        codes, vals, sp = R.finite_codes(fmt)
        assert len(codes) == n and sp.tolist() == special and np.isfinite(vals).all()
        assert sorted(codes.tolist() + sp.tolist()) == list(range(n + len(special)))
        allv = R.all_code_values(fmt)
        half = len(allv) // 2
        table = code_table(fmt)                                    # the non-negative finite codes of tests/mx_reference.py
        assert np.array_equal(allv[:len(table)], table) and np.array_equal(allv[half:half + len(table)], -table)
        assert np.signbit(allv[half]) and allv[half] == 0 and not np.signbit(allv[0])           # both zeros
        if fmt == "mxfp4":
            assert allv.tolist() == list(ops._FP4_VALUES) and np.array_equal(np.signbit(allv), np.signbit(np.array(ops._FP4_VALUES)))
        else:
            t = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(R._F8[fmt]).double().numpy()
            assert np.array_equal(np.isnan(t), np.isnan(allv)) and np.array_equal(t[~np.isnan(t)], allv[~np.isnan(t)])
            assert np.array_equal(np.signbit(t), np.signbit(allv))
        sub = R.subnormal_codes(fmt)
        assert len(sub) == {"mxfp4": 2, "mxfp8_e4m3": 14, "mxfp8_e5m2": 6}[fmt] and (np.abs(allv[sub]) < np.abs(allv[sub.max() % half + 1])).all()
        assert allv[R.code_of(fmt, 1.5)] == 1.5 and allv[R.code_of(fmt, -1.0)] == -1.0


def test_dense_is_dequantize():
    rng = np.random.default_rng(1)
    for fmt in R.GEMM_FMTS:
        codes = rng.choice(R.finite_codes(fmt)[0], size=(9, 256))
        scales = rng.integers(0, 239, size=(9, 8)).astype(np.uint8)     # (element * 2^127 can exceed fp32: dequantize() to float32 gives Inf there)
        codes[0], scales[0, :4] = R.code_of(fmt, -1.5), (0, 1, 254, 253)
        want = export_from_codes(codes, scales, fmt).dequantize().double().numpy()
        got = R.dense(codes, scales, fmt)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        scales[3, 5] = 0xFF
        assert np.isnan(R.dense(codes, scales, fmt)[3, 160:192]).all() and not np.isnan(R.dense(codes, scales, fmt)[3, :160]).any()


def test_window_operand_integers_are_the_values():
    rng = np.random.default_rng(2)
    for name, (fmt, codes) in R.WINDOWS.items():
        sc = (119, 121, 124)
        e, ints = R.window_operand(rng, 5, 256, fmt, codes, sc)
        q = R.window_quantum(fmt, codes, sc)
        assert torch.equal(e.dequantize().double(), torch.from_numpy(ints.astype(np.float64) * q)), name
        got = np.unique(e.elements.numpy() & 0xF if fmt == "mxfp4" else e.elements.numpy())
        assert set(got.tolist()) <= set(codes) and len(got) >= min(len(set(codes)), 14)
        assert set(np.unique(e.scales.numpy()).tolist()) == set(sc)
        assert np.abs(ints).min() == 0 or np.abs(ints).min() >= 4                   # the quantum is the largest one
    assert R.quantum([96.0, 448.0, 64.0]) == 32.0 and R.quantum([0.0, 0.375]) == 0.125
    # the case checked in the issue: the E4M3 top binade is 8 .. 14 after scaling, and against the full FP4 grid with one shared scale the
    # sum |a| * max |w| bound stays below 2^24 up to K = 28672
    fmt, codes = R.WINDOWS["e4m3_top1"]
    for K in (4096, 11008, 28672):
        _, ai = R.window_operand(rng, 16, K, fmt, codes, (127,))
        _, wi = R.window_operand(rng, 8, K, *R.WINDOWS["fp4_full"], (127,))
        assert sorted(set(np.abs(ai).reshape(-1).tolist())) == list(range(8, 15)) and np.abs(wi).max() == 12
        assert prove_exact(ai, wi) <= K * 14 * 12 < 2 ** 24


def _sum_cases():
    for name, fam in R.SHORT_SUMS.items():
        for K in R.SHORT_K:
            for i, (M, N) in enumerate(R.SUM_SHAPES):
                yield f"{name} K={K} M={M}", fam, M, N, K, 1000 * K + i
    for name, fam in R.LONG_SUMS.items():
        for K in R.LONG_K:
            for i, (M, N) in enumerate(R.LONG_SHAPES):
                yield f"{name} K={K} M={M}", fam, M, N, K, 1000 * K + i


def test_every_sum_family_passes_the_exactness_proof():
    """the gate of test_gpu_mx_gemm_codes.py's sum cases, on the operands those tests draw (same seeds)"""
    worst = 0
    for what, fam, M, N, K, seed in _sum_cases():
        ac, asc, a_fmt, wc, wsc, w_fmt, q, ai, wi = R.sum_case(fam, M, N, K, seed)
        bound = prove_exact(ai, wi)
        worst = max(worst, bound)
        ref = R.dense(ac, asc, a_fmt) @ R.dense(wc, wsc, w_fmt).T
        assert np.array_equal(ref, (ai @ wi.T).astype(np.float64) * q), what
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), what
    print(f"[mx_gemm exact sums] largest proved bound {worst} = {worst / 2 ** 24:.3f} * 2^24")
    for fam in list(R.SHORT_SUMS.values()) + list(R.LONG_SUMS.values()):              # scale sets wider than {127, 128}
        assert set(fam[1]) | set(fam[3]) != {127, 128} and (len(fam[1]) > 1 or len(fam[3]) > 1)
    with pytest.raises(AssertionError):                                                # and the gate does reject a window that is too wide
        R.sum_case(("e4m3_top", (120, 128), "e5m2_top", (127, 130)), 13, 52, 28672, 0)


def test_single_product_families_cover_every_code_and_scale_byte():
    for fmt in R.GEMM_FMTS:
        fin = set(R.finite_codes(fmt)[0].tolist())
        hot, hs = R.hot_code_rows(fmt, 1)
        assert ((hot != 0).sum(1) <= 1).all() and set(hot.max(1).tolist()) | {0} == fin | {0}
        ks = np.array([np.flatnonzero(r)[0] for r in hot if r.any()])
        assert set(ks.tolist()) == set(range(256))                    # every position of two K steps
        assert len(np.unique(hs, axis=0)) > 16 and (np.diff(hs.astype(int), axis=1) != 0).any(1).all()     # scales differ per row and block
        fill, _ = R.fill_code_rows(fmt, 2)
        assert (fill == fill[:, :1]).all() and set(fill[:, 0].tolist()) == fin and fill.shape[0] > 32
        sb, ss = R.scale_byte_rows(fmt)
        seen = set()
        for r in range(1020):
            (k,) = np.flatnonzero(sb[r])
            blk = k // 32
            seen.add((int(ss[r, blk]), blk % 4))
            assert (np.delete(ss[r], blk) != ss[r, blk]).all() and (ss[r] != 0xFF).all()
        assert seen == {(b, g) for b in range(255) for g in range(4)}
        pc, ps = R.scale_partner_rows(fmt)
        assert np.isin(pc, list(fin)).all() and (R.dense(pc, ps, fmt) != 0).all() and not np.isin(pc, R.subnormal_codes(fmt)).all()
        if fmt != "mxfp4":
            sp, _ = R.special_code_rows(fmt)
            assert sorted(sp.max(1).tolist()) == R.finite_codes(fmt)[2].tolist() and ((sp != 0).sum(1) == 1).all()


@pytest.mark.parametrize("fmt", ["mxfp8_e4m3", "mxfp8_e5m2"])
def test_reference_export_never_emits_a_special_code(fmt):
    """tests/mx_reference.py's export over every 16-bit input pattern (the GPU test asserts the same of ops.mx_export)"""
    from test_gpu_mx import exhaustive_bits
    sp = R.finite_codes(fmt)[2]
    for dtype in ("bf16", "fp16"):
        codes, scales = export_bits(exhaustive_bits(dtype), dtype, fmt)
        assert not np.isin(codes, sp).any()
        assert (codes.reshape(-1, 32)[scales == 0xFF] == 0).all()
        used = np.unique(codes)
        print(f"[mx export codes] {fmt} from every {dtype} pattern: {len(used)} of {len(R.finite_codes(fmt)[0])} finite codes emitted")


# seeded faults: each is a way a kernel could be subtly wrong; applied to the reference operands, it must change at least one output that the
# family's GPU test compares.  (a_dense, w_dense) -> faulty (a_dense, w_dense) or None where the family holds nothing the fault touches.
def _table_fault(kind, fmt, present, rng):
    t = R.all_code_values(fmt).copy()
    fin = R.finite_codes(fmt)[0]
    half = len(t) // 2
    if kind == "lsb":
        cand = [c for c in present if c in set(fin.tolist()) and (c ^ 1) in set(fin.tolist())]
        c = int(rng.choice(cand))
        t[c] = R.all_code_values(fmt)[c ^ 1]
    elif kind == "subnormal":
        sub = R.subnormal_codes(fmt)
        if not np.isin(present, sub).any():
            return None
        t[sub] = 0.0
    elif kind == "top":
        top = int(fin[fin < half].max())
        if not np.isin(present, [top, top + half]).any():
            return None
        t[top], t[top + half] = t[top - 1], t[top - 1 + half]
    return t


FAULTS = ("lsb", "subnormal", "top", "scale+1 g0", "scale+1 g1", "scale+1 g2", "scale+1 g3", "scale 0 as 1", "k swap", "step dropped")


def _apply_fault(fault, codes, scales, fmt, rng):
    """-> the operand's dense values under the fault, or None if the operand holds nothing it touches"""
    K = codes.shape[1]
    if fault in ("lsb", "subnormal", "top"):
        t = _table_fault(fault, fmt, np.unique(codes), rng)
        return None if t is None else R.dense(codes, scales, fmt, t)
    if fault.startswith("scale+1"):
        g = int(fault[-1])
        s = scales.astype(np.int64)
        s[:, g::4] = np.where(s[:, g::4] < 254, s[:, g::4] + 1, 253)
        return R.dense(codes, s.astype(np.uint8), fmt)
    if fault == "scale 0 as 1":
        if not (scales == 0).any():
            return None
        return R.dense(codes, np.where(scales == 0, 1, scales).astype(np.uint8), fmt)
    d = R.dense(codes, scales, fmt)
    if fault == "k swap":      # two k of one K step, in different scale blocks (within a block a one-hot row meets the same fill code: the
        s = int(rng.integers(0, K // 128))        # parent's layout test, whose partner differs along k, owns that case)
        g1, g2 = rng.choice(4, size=2, replace=False)
        k1, k2 = 128 * s + 32 * g1 + int(rng.integers(0, 32)), 128 * s + 32 * g2 + int(rng.integers(0, 32))
        d[:, [k1, k2]] = d[:, [k2, k1]]
        return d
    if fault == "step dropped":
        if K // 128 <= 32:
            return None
        s = int(rng.integers(32, K // 128))
        d[:, 128 * s:128 * (s + 1)] = 0.0
        return d
    raise AssertionError(fault)


def _changes(a, w, a2, w2, compared=None):
    """does any compared output differ?  (single products and proved-exact sums: float64 holds every value exactly, so != is exact)"""
    with np.errstate(over="ignore", invalid="ignore"):
        diff = (a @ w.T) != (a2 @ w2.T)
    return bool((diff if compared is None else diff & compared).any())


def _families():
    """name, (a_codes, a_scales, a_fmt, w_codes, w_scales, w_fmt), mask of the outputs the GPU test compares exactly (None: all)"""
    for a_fmt, w_fmt in R.PAIRS:
        yield f"code table {a_fmt} x {w_fmt} hot a", (*R.hot_code_rows(a_fmt, 1), a_fmt, *R.fill_code_rows(w_fmt, 2), w_fmt), None
        yield f"code table {a_fmt} x {w_fmt} hot w", (*R.fill_code_rows(a_fmt, 3), a_fmt, *R.hot_code_rows(w_fmt, 4), w_fmt), None
    for a_fmt, w_fmt in R.PAIRS:
        for hot in "aw":
            ops_ = (*R.scale_byte_rows(a_fmt), a_fmt, *R.scale_partner_rows(w_fmt), w_fmt) if hot == "a" else \
                   (*R.scale_partner_rows(a_fmt), a_fmt, *R.scale_byte_rows(w_fmt), w_fmt)
            ref = R.dense(*ops_[:3]) @ R.dense(*ops_[3:]).T
            yield f"scale bytes {a_fmt} x {w_fmt} hot {hot}", ops_, R.normal_or_zero(torch.from_numpy(ref)).numpy() & (ref != 0)
    for what, fam, M, N, K, seed in _sum_cases():
        c = R.sum_case(fam, M, N, K, seed)
        yield "sums " + what, c[:6], None


def test_seeded_faults_change_an_output_of_every_family_they_touch():
    """Every fault, applied to A and to W of every new exact family that holds what the fault touches (a family without sub-normal codes
    cannot notice them read as zero; only K > 4096 has a step 32): at least one compared output changes.  The code table is held to
    more: a mantissa LSB flipped in ANY finite code, in either operand, changes an output."""
    caught = {f: 0 for f in FAULTS}
    for name, (ac, asc, a_fmt, wc, wsc, w_fmt), compared in _families():
        rng = np.random.default_rng(len(name) * 7919 + ac.shape[0])
        a, w = R.dense(ac, asc, a_fmt), R.dense(wc, wsc, w_fmt)
        single = not name.startswith("sums")
        for fault in FAULTS:
            for side in "aw":
                codes, scales, fmt = (ac, asc, a_fmt) if side == "a" else (wc, wsc, w_fmt)
                if name.startswith("code table") and fault == "lsb":     # the code table must notice the fault on EVERY finite code
                    fin = R.finite_codes(fmt)[0]
                    for c in fin:
                        t = R.all_code_values(fmt).copy()
                        if (c ^ 1) not in fin:
                            continue
                        t[c] = R.all_code_values(fmt)[c ^ 1]
                        bad = R.dense(codes, scales, fmt, t)
                        assert _changes(a, w, bad if side == "a" else a, bad if side == "w" else w), (name, fault, side, hex(c))
                    caught[fault] += 1
                    continue
                bad = _apply_fault(fault, codes, scales, fmt, rng)
                if bad is None:
                    continue
                if single and fault == "k swap" and not (bad != (a if side == "a" else w)).any():
                    continue                                               # the swap met two equal elements (same code, same scale)
                assert _changes(a, w, bad if side == "a" else a, bad if side == "w" else w, compared), (name, fault, side)
                caught[fault] += 1
    print("[mx_gemm seeded faults] (family, operand) pairs that noticed each fault:", caught)
    assert all(n > 0 for n in caught.values()), caught
    assert caught["scale 0 as 1"] >= 18 and caught["step dropped"] >= 2 * len(R.LONG_SUMS) * len(R.LONG_K) * len(R.LONG_SHAPES)


def test_what_the_same_faults_do_to_the_bounded_tier():
    """For the record (printed, not asserted): max |delta| / (2^-24 S) of the Gaussian tier's reference under the decode faults above,
    against the tier's bound 2 K.  A fault below the bound is one the bounded tier cannot notice."""
    from test_gpu_mx import to_bits
    for a_fmt in ("mxfp8_e4m3", "mxfp8_e5m2"):
        for K in (4096, 11008):
            g = torch.Generator().manual_seed(K)
            x, wt = torch.randn(16, K, generator=g), torch.randn(384, K, generator=g) * 0.05
            ac, asc = export_bits(x.numpy().view(np.uint32), "fp32", a_fmt)
            wc, wsc = export_bits(wt.numpy().view(np.uint32), "fp32", "mxfp4")
            ac, asc, wc, wsc = ac.reshape(16, K), asc.reshape(16, K // 32), wc.reshape(384, K), wsc.reshape(384, K // 32)
            a, w = R.dense(ac, asc, a_fmt), R.dense(wc, wsc, "mxfp4")
            ref, S = a @ w.T, np.abs(a) @ np.abs(w).T
            t_lsb = R.all_code_values(a_fmt)
            t_lsb = np.where(np.isfinite(t_lsb[np.arange(256) ^ 1]), t_lsb[np.arange(256) ^ 1], t_lsb)
            one_col = a.copy()
            one_col[:, 77] = t_lsb[ac[:, 77]] * np.exp2(asc[:, 77 // 32].astype(np.float64) - 127)
            rng = np.random.default_rng(0)
            faulty = {"mantissa LSB flipped in one k column": one_col,
                      "largest finite code read as the one below": _apply_fault("top", ac, asc, a_fmt, rng),
                      "all sub-normal codes read as zero": _apply_fault("subnormal", ac, asc, a_fmt, rng),
                      "scale byte + 1 in block position 2": _apply_fault("scale+1 g2", ac, asc, a_fmt, rng),
                      "two k swapped": _apply_fault("k swap", ac, asc, a_fmt, rng),
                      "K step 5 dropped": np.concatenate([a[:, :640], np.zeros((16, 128)), a[:, 768:]], 1)}
            for what, bad in faulty.items():
                if bad is None:
                    print(f"[bounded tier under a fault] A {a_fmt} K={K}: {what}: no such code in the export")
                    continue
                ratio = (np.abs(bad @ w.T - ref) / (2.0 ** -24 * S)).max()
                print(f"[bounded tier under a fault] A {a_fmt} K={K}: {what}: max |delta| / (2^-24 S) = {ratio:.0f} vs bound {2 * K}"
                      f" -> {'caught' if ratio > 2 * K else 'MISSED'}")


def test_bias_of_another_dtype_would_promote_the_sum():
    """why MXLinear casts its bias to the activation's dtype: fp16 + bf16 promotes to fp32, and the output dtype must follow x"""
    assert (torch.zeros(2, dtype=torch.float16) + torch.zeros(2, dtype=torch.bfloat16)).dtype == torch.float32
    m = MXLinear(256, 64, bias=True, dtype=torch.bfloat16)
    src = open(os.path.join(ROOT, "llm-qat_amd", "mx_inference.py")).read()
    assert "self.bias.to(y.dtype)" in src and m.bias.dtype == torch.bfloat16
