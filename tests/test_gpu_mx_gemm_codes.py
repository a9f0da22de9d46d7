"""The MX GEMM's exact tier over the whole operand space (tests/test_gpu_mx_gemm.py feeds the instruction FP4-grid magnitudes, FP8 codes
8 .. 107 and scale bytes 118 .. 134 only): every finite element code of every format and every scale byte 0 .. 254 through the
instruction in both operand positions and on both launch routes, the special codes, products outside fp32's normal range, sums over the
codes real exports hold (proved exactly summable in int64 first), K = 128 .. 28672, the copy route of mx_matmul_tensors, and MXLinear's
host paths.  Everything but the MXLinear GEMM itself is compared bit for bit with MXExport.dequantize() in float64; the only relaxation
is that a zero result matches a zero of either sign.  tests/test_mx_gemm_cpu.py proves on the CPU that these cases notice a decode or
scale fault of one mantissa step, which the bounded tier cannot."""
import numpy as np
import pytest
import torch
from torch import nn

import llm_qat_amd
from llm_qat_amd import MXLinear, ops
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_gemm_reference as R
from mx_gemm_reference import PAIRS, export_from_codes, ref64, to_cpu, to_device

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
FP8 = ("mxfp8_e4m3", "mxfp8_e5m2")


def run(a, w, route=None):
    """fp32 result on the CPU; route: the launch shape stats() must report"""
    llm_qat_amd.stats(reset=True)
    out = ops.mx_matmul(to_device(a), to_device(w), out_dtype=torch.float32).cpu()
    if route is not None:
        st = llm_qat_amd.stats()
        other = "mx_gemm_tiled" if route == "mx_gemm_skinny" else "mx_gemm_skinny"
        assert st.get(route) == 1 and st.get("mx_gemm_launch") == 1 and other not in st, st
    return out


def assert_exact(out, ref, where=None):
    """out == ref bit for bit (ref must be an fp32 value), a zero of either sign for a zero; where: the outputs to compare"""
    want = ref.to(torch.float32)
    sel = torch.ones_like(want, dtype=torch.bool) if where is None else where
    assert want.double()[sel].equal(ref[sel]), "the reference itself is not an fp32 value"
    out = out.reshape(want.shape)
    same = (out.view(torch.int32) == want.view(torch.int32)) | ((want == 0) & (out == 0))
    bad = torch.nonzero(sel & ~same)
    assert bad.numel() == 0, (f"{bad.shape[0]} of {int(sel.sum())} differ, first at {bad[:4].tolist()}: got {out[tuple(bad[0])].item()!r}, "
                              f"want {want[tuple(bad[0])].item()!r}")


def _sliced(codes, scales, fmt, rows=32):
    for r0 in range(0, codes.shape[0], rows):
        yield r0, export_from_codes(codes[r0:r0 + rows], scales[r0:r0 + rows], fmt)


def _both_routes(ac, asc, a_fmt, w, check):
    """the whole A on the tiled kernel, then 32 rows of A at a time on the skinny one; check(out, first row, rows)"""
    assert ac.shape[0] > 32
    check(run(export_from_codes(ac, asc, a_fmt), w, "mx_gemm_tiled"), 0, ac.shape[0])
    for r0, sub in _sliced(ac, asc, a_fmt):
        check(run(sub, w, "mx_gemm_skinny"), r0, sub.shape[0])


# ---- the code table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hot", ["a", "w"])
@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_every_finite_code_is_decoded_to_its_ocp_value(a_fmt, w_fmt, hot):
    """One operand one-hot per row (row i: the i-th finite code at a k that walks over two K steps), the other with every row filled with
    one finite code: out[m, n] is one product of two at most 4-bit significands, exact in fp32.  After both values of `hot` every finite
    code of both formats has been the instruction's A and its B operand, against every finite code of the other format."""
    if hot == "a":
        (ac, asc), (wc, wsc) = R.hot_code_rows(a_fmt, 1), R.fill_code_rows(w_fmt, 2)
    else:
        (ac, asc), (wc, wsc) = R.fill_code_rows(a_fmt, 3), R.hot_code_rows(w_fmt, 4)
    w = export_from_codes(wc, wsc, w_fmt)
    ref, _ = ref64(export_from_codes(ac, asc, a_fmt), w)
    assert torch.isfinite(ref).all() and R.normal_or_zero(ref).all()
    live = lambda c, s, f: int((R.dense(c, s, f) != 0).any(1).sum())        # rows that carry a nonzero code: all but the two zeros'
    assert int((ref != 0).sum()) == live(ac, asc, a_fmt) * live(wc, wsc, w_fmt)
    _both_routes(ac, asc, a_fmt, w, lambda out, r0, n: assert_exact(out, ref[r0:r0 + n]))


# ---- the special codes -----------------------------------------------------------------------------------------------------------------
def _has_special(elements, fmt):
    sp = torch.from_numpy(R.finite_codes(fmt)[2].astype(np.int64))
    return torch.isin(elements.cpu().long(), sp).any().item()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("fmt", FP8)
def test_export_never_emits_a_special_code(fmt, dtype):
    """over every 16-bit input pattern (the blocks test_gpu_mx.py builds: NaN and Inf inputs included, which become 0xFF scale blocks
    with codes 0)"""
    from test_gpu_mx import exhaustive_bits, from_bits
    e = ops.mx_export(from_bits(exhaustive_bits(dtype), dtype), fmt)
    assert not _has_special(e.elements, fmt)
    x = torch.tensor([3e38, -3e38, 65504.0, 1e30, 448.0, 57344.0, 500.0, 61440.0] * 4, device="cuda").repeat(4, 1)   # fp32, at the top of the range
    assert not _has_special(ops.mx_export(x, fmt).elements, fmt)


@pytest.mark.parametrize("hot", ["a", "w"])
@pytest.mark.parametrize("fmt", FP8)
@pytest.mark.parametrize("other", R.GEMM_FMTS)
def test_special_codes_behave_as_documented(fmt, other, hot):
    """Each special code once as the single nonzero of a row, against rows of +-1 and one row of zeros.  The IEEE value of dequantize()
    is NaN for a NaN code, +-Inf (times the sign of the partner) for an E5M2 Inf code, and NaN for Inf x 0.  Measured on MI355X: the
    instruction gives exactly these."""
    sc, ssc = R.special_code_rows(fmt)
    if hot == "a":
        pad = np.zeros((40 - len(sc), R.TABLE_K), np.uint8), np.full((40 - len(sc), R.TABLE_K // 32), 127, np.uint8)
        ac, asc, a_fmt = np.concatenate([sc, pad[0]]), np.concatenate([ssc, pad[1]]), fmt          # 40 rows: the tiled route
        (wc, wsc), w_fmt = R.ones_rows(other, 24), other
    else:
        (ac, asc), a_fmt = R.ones_rows(other, 40), other
        wc, wsc, w_fmt = sc, ssc, fmt
    w = export_from_codes(wc, wsc, w_fmt)
    ref, _ = ref64(export_from_codes(ac, asc, a_fmt), w)
    vals = torch.from_numpy(R.all_code_values(fmt)[R.finite_codes(fmt)[2]])
    n = len(vals)
    hit = ref[:n] if hot == "a" else ref[:, :n].T                        # [special code, partner row]; the last partner row is zeros
    assert torch.equal(torch.isnan(hit[:, :-1]), torch.isnan(vals)[:, None].expand_as(hit[:, :-1]))
    assert torch.equal(torch.isinf(hit[:, :-1]), torch.isinf(vals)[:, None].expand_as(hit[:, :-1])) and torch.isnan(hit[:, -1]).all()
    inf = torch.isinf(vals)
    assert torch.equal(hit[inf, 0], vals[inf]) and torch.equal(hit[inf, 1], -vals[inf])          # against +1 and against -1

    def check(out, r0, rows):
        want = ref[r0:r0 + rows].to(torch.float32)
        out = out.reshape(want.shape)
        assert torch.equal(torch.isnan(out), torch.isnan(want)), f"NaN positions differ: got {out[:n, :4]}, want {want[:n, :4]}"
        ok = ~torch.isnan(want)
        assert torch.equal(out[ok], want[ok]), f"got {out[:n, :4]}, want {want[:n, :4]}"

    _both_routes(ac, asc, a_fmt, w, check)


# ---- the scale bytes -------------------------------------------------------------------------------------------------------------------
def _scale_case(a_fmt, w_fmt, hot):
    if hot == "a":
        (ac, asc), (wc, wsc) = R.scale_byte_rows(a_fmt), R.scale_partner_rows(w_fmt)
    else:
        (ac, asc), (wc, wsc) = R.scale_partner_rows(a_fmt), R.scale_byte_rows(w_fmt)
    w = export_from_codes(wc, wsc, w_fmt)
    ref, _ = ref64(export_from_codes(ac, asc, a_fmt), w)
    by_byte = ref if hot == "a" else ref.T                                # [1020 (byte, block position), 255 partners]
    return ac, asc, w, ref, by_byte


@pytest.mark.parametrize("hot", ["a", "w"])
@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_every_scale_byte_in_every_block_position(a_fmt, w_fmt, hot):
    """Scale byte b = 0 .. 254 in each of the four block positions of a K step, over a single 1.5, with seven decoy bytes in the row's
    other blocks, against 255 partner rows whose own bytes are near 254 - n: every (byte, position) meets at least 100 partners with
    which the one product is a normal fp32 value, and those must be exact.  Pins byte 0 = 2^-127, byte 254 = 2^127 and the lane to scale
    byte mapping over the whole range."""
    ac, asc, w, ref, by_byte = _scale_case(a_fmt, w_fmt, hot)
    normal = R.normal_or_zero(ref) & (ref != 0)
    per = (normal if hot == "a" else normal.T).sum(1)
    assert per.shape == (1020,) and int(per.min()) >= 100, int(per.min())
    _both_routes(ac, asc, a_fmt, w, lambda out, r0, n: assert_exact(out, ref[r0:r0 + n], normal[r0:r0 + n]))


@pytest.mark.parametrize("hot", ["a", "w"])
@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_products_outside_the_normal_range_round_once(a_fmt, w_fmt, hot):
    """The same operands, the other outputs: single products whose exact value is an fp32 sub-normal, below half the smallest one, or
    above the fp32 maximum.  Expected: the float64 reference rounded once to fp32 (gradual underflow, ties to even; +-Inf above the
    maximum)."""
    ac, asc, w, ref, _ = _scale_case(a_fmt, w_fmt, hot)
    outside = ~R.normal_or_zero(ref)
    want = ref.to(torch.float32)
    assert int((outside & torch.isinf(want)).sum()) > 1000 and int((outside & (want == 0)).sum()) > 1000
    sub = outside & (want != 0) & ~torch.isinf(want)
    assert int(sub.sum()) > 1000 and int((sub & (want.double() != ref)).sum()) > 100        # sub-normal results, many of them rounded

    def check(out, r0, rows):
        o, wnt, sel = out.reshape(rows, -1), want[r0:r0 + rows], outside[r0:r0 + rows]
        same = (o.view(torch.int32) == wnt.view(torch.int32)) | ((wnt == 0) & (o == 0))
        bad = torch.nonzero(sel & ~same)
        assert bad.numel() == 0, (f"{bad.shape[0]} of {int(sel.sum())} differ, first at {bad[:4].tolist()}: got {o[tuple(bad[0])].item()!r}, "
                                  f"want {wnt[tuple(bad[0])].item()!r} (exact {ref[r0:r0 + rows][tuple(bad[0])].item()!r})")

    _both_routes(ac, asc, a_fmt, w, check)


# ---- sums over the codes real exports use ----------------------------------------------------------------------------------------------
def _sum_check(family, M, N, K, seed):
    ac, asc, a_fmt, wc, wsc, w_fmt, q, ai, wi = R.sum_case(family, M, N, K, seed)       # prove_exact runs inside, before the launch
    a, w = export_from_codes(ac, asc, a_fmt), export_from_codes(wc, wsc, w_fmt)
    ref, _ = ref64(a, w)
    assert torch.equal(ref, torch.from_numpy((ai @ wi.T).astype(np.float64) * q))      # the proof's integers are the operands' values
    assert_exact(run(a, w, "mx_gemm_skinny" if M <= 32 else "mx_gemm_tiled"), ref)


@pytest.mark.parametrize("K", R.SHORT_K)
@pytest.mark.parametrize("name", list(R.SHORT_SUMS))
def test_exact_sums_over_export_code_windows(name, K):
    """K = 128 (one step: seven idle waves on the skinny route, the tiled kernel's tail alone), 384 (three steps) and 1408, on both
    skinny instantiations and the tiled kernel, tails in M and N"""
    for i, (M, N) in enumerate(R.SUM_SHAPES):
        _sum_check(R.SHORT_SUMS[name], M, N, K, 1000 * K + i)


@pytest.mark.parametrize("K", R.LONG_K)
@pytest.mark.parametrize("name", list(R.LONG_SUMS))
def test_exact_sums_long_k_skinny(name, K):
    """86 and 224 K steps on the skinny route: up to seven trips of each wave's outer loop, with the re-loaded steps past the end"""
    for i, (M, N) in enumerate(R.LONG_SHAPES):
        _sum_check(R.LONG_SUMS[name], M, N, K, 1000 * K + i)


# ---- the copy route --------------------------------------------------------------------------------------------------------------------
def _misaligned(t):
    """the same bytes at an odd address"""
    buf = torch.empty(t.numel() + 64, dtype=torch.uint8, device=t.device)
    off = 1 if buf.data_ptr() % 2 == 0 else 2
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


def _column_slice(t):
    """the same bytes as a column slice of a wider tensor: not contiguous"""
    wide = torch.full((t.shape[0], t.shape[1] + 5), 0xFF, dtype=torch.uint8, device=t.device)
    v = wide[:, 3:3 + t.shape[1]]
    v.copy_(t)
    assert not v.is_contiguous() or t.shape[0] == 1
    return v


@pytest.mark.parametrize("M", [20, 150])
@pytest.mark.parametrize("a_fmt,w_fmt", [("mxfp8_e4m3", "mxfp4"), ("mxfp4", "mxfp8_e5m2")])
def test_misaligned_and_strided_operands_give_the_aligned_result(a_fmt, w_fmt, M):
    rng = np.random.default_rng(M)
    a, ai = R.grid_operand(rng, M, 512, a_fmt)
    w, wi = R.grid_operand(rng, 77, 512, w_fmt)
    R.prove_exact(ai, wi)
    a, w = to_device(a), to_device(w)
    base = ops.mx_matmul(a, w, out_dtype=torch.float32)
    assert_exact(base.cpu(), ref64(to_cpu(a), to_cpu(w))[0])
    for which in ("elements", "scales"):
        for make in (_misaligned, _column_slice):
            for side in ("a", "w"):
                ops_ = {"a": ops.MXExport(a.elements, a.scales, a.fmt, a.shape, a.dtype), "w": ops.MXExport(w.elements, w.scales, w.fmt, w.shape, w.dtype)}
                setattr(ops_[side], which, make(getattr(ops_[side], which)))
                llm_qat_amd.stats(reset=True)
                out = ops.mx_matmul(ops_["a"], ops_["w"], out_dtype=torch.float32)
                assert llm_qat_amd.stats().get("mx_gemm_launch") == 1
                assert torch.equal(out.view(torch.int32), base.view(torch.int32)), (which, make.__name__, side)


# ---- MXLinear's host paths -------------------------------------------------------------------------------------------------------------
def _mx_linear(i, o, dtype, bias, seed=0):
    torch.manual_seed(seed)
    layer = QuantizeLinear(i, o, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3").to("cuda", dtype)
    with torch.no_grad():
        layer.weight.normal_(0, 0.02)
    if bias:                                   # (the constructor ignores `bias`, as the reference's does: a bias is assigned afterwards)
        layer.bias = nn.Parameter(torch.randn(o, device="cuda", dtype=dtype) * 0.5)
    return layer.eval(), MXLinear.from_quantize_linear(layer)


def _check_module(mxl, layer, x):
    """out32 = the fp32 GEMM over the same exports, held to the float64 reference under the 2 K bound; the module's output must then be
    out32 rounded once to x's dtype, plus the bias (rounded to that dtype), in that dtype's arithmetic -- bit for bit"""
    K, N = layer.in_features, layer.out_features
    xc = x.contiguous()
    a = ops.mx_export(xc, layer.act_format)
    wexp = ops.mx_export(layer.weight.detach(), layer.weight_format)
    assert torch.equal(wexp.elements, mxl.weight_elements) and torch.equal(wexp.scales, mxl.weight_scales)
    out32 = ops.mx_matmul(a, wexp, out_dtype=torch.float32)
    ref, S = ref64(to_cpu(a), to_cpu(wexp))
    ratio = ((out32.cpu().double().reshape(ref.shape) - ref).abs() / (U * S).clamp_min(1e-300)).max().item()
    print(f"[MXLinear {tuple(x.shape)} {x.dtype}] max |out32 - ref| / (2^-24 S) = {ratio:.4f}  (bound {2 * K})")
    assert ratio <= 2 * K
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        y = mxl(x)
    st = llm_qat_amd.stats()
    assert st.get("mx_export_launch") == 1 and st.get("mx_gemm_launch") == 1
    assert y.dtype == x.dtype and y.shape == x.shape[:-1] + (N,)
    want = out32.to(x.dtype)
    if mxl.bias is not None:
        want = want + mxl.bias.to(x.dtype)
    assert want.dtype == x.dtype
    it = torch.int32 if x.dtype == torch.float32 else torch.int16
    assert torch.equal(y.contiguous().view(it), want.reshape(y.shape).view(it))
    return y


@pytest.mark.parametrize("shape", [(2, 24), (3, 1000), (7,)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_linear_with_bias_and_leading_dimensions(dtype, shape):
    layer, mxl = _mx_linear(512, 200, dtype, bias=True)
    assert mxl.bias is not None and mxl.bias.dtype == dtype and torch.equal(mxl.bias, layer.bias)
    x = torch.randn(*shape, 512, device="cuda", dtype=dtype)
    y = _check_module(mxl, layer, x)
    _, bare = _mx_linear(512, 200, dtype, bias=False)
    with torch.no_grad():
        assert not torch.equal(y, bare(x))                                # the bias took part


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("xdtype", [torch.float16, torch.float32, torch.bfloat16])
def test_mx_linear_output_dtype_follows_the_activation(xdtype, bias):
    layer, mxl = _mx_linear(384, 136, torch.bfloat16, bias=bias, seed=1)
    for shape in ((5, 384), (2, 24, 384)):
        _check_module(mxl, layer, torch.randn(*shape, device="cuda", dtype=xdtype))


@pytest.mark.parametrize("bias", [False, True])
def test_mx_linear_non_contiguous_activation(bias):
    layer, mxl = _mx_linear(256, 72, torch.bfloat16, bias=bias, seed=2)
    big = torch.randn(2, 40, 512, device="cuda", dtype=torch.bfloat16)
    for x in (big[..., ::2], big[..., 256:], big.transpose(0, 1)[..., :256]):
        assert not x.is_contiguous()
        y = _check_module(mxl, layer, x)
        with torch.no_grad():
            assert torch.equal(y, mxl(x.contiguous()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", [(0,), (0, 7), (3, 0)])
def test_mx_linear_zero_tokens(shape, bias):
    layer, mxl = _mx_linear(256, 72, torch.bfloat16, bias=bias)
    x = torch.empty(*shape, 256, device="cuda", dtype=torch.bfloat16)
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        y = mxl(x)
    st = llm_qat_amd.stats()
    assert y.shape == shape + (72,) and y.dtype == torch.bfloat16 and y.numel() == 0 and y.device == x.device
    assert "mx_gemm_launch" not in st and "mx_gemm_skinny" not in st and "mx_gemm_tiled" not in st and "mx_export_launch" not in st
