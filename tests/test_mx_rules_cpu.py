"""Scale rule and saturation-masked gradient of the MX quantizer, CPU tier (no GPU): worked values of the numpy reference
(tests/mx_rules_reference.py), its floor rule against tests/mx_reference.py over every bf16 pattern, the no-saturation property of the ceil
rule over every bf16 / fp16 pattern, the sensitivity of the GPU tier's cases to deliberately wrong references, the argument errors of every
new keyword, the validation codes of the three new entry points (validation comes before any launch), and the public signatures."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, ops
from llm_qat_amd.mx_inference import MXLinear
from llm_qat_amd.utils_quant import QuantizeLinear

import mx_reference as M
import mx_rules_reference as R
from mx_reference import decode, encode, params
from mx_rot_reference import rotate_values
from mx_rules_cases import EXPORT_FMTS, FMTS, exhaustive_bits, grad_bits, lead_bits, rand_bits


def block_led_by(lead, dtype="bf16"):
    v = np.array([lead, 1.0, -3.0, 0.25] + [0.5] * 28)
    return encode(v, dtype).reshape(1, 32)


# ---- worked literals ---------------------------------------------------------------------------------------------------------------------

def test_worked_fp4_block_led_by_seven():
    b = block_led_by(7.0)
    assert R.shared_exp(np.array([7.0]), "mxfp4", "floor").tolist() == [0]
    y = decode(R.quantize_bits(b, "bf16", "mxfp4", "floor"), "bf16")[0]
    assert y[0] == 6.0 and y[1] == 1.0 and y[2] == -3.0
    keep = R.keep_mask(b, "bf16", "mxfp4", "floor")[0]
    assert keep.tolist() == [False] + [True] * 31
    assert R.pack_mask(keep).tolist() == [0xFE, 0xFF, 0xFF, 0xFF]
    assert R.shared_exp(np.array([7.0]), "mxfp4", "ceil").tolist() == [1]
    yc = decode(R.quantize_bits(b, "bf16", "mxfp4", "ceil"), "bf16")[0]
    assert yc[0] == 8.0 and yc[1] == 1.0 and yc[2] == -3.0 and yc[3] == 0.0     # t = 3.5 -> 4 (tie to even), 0.5, -1.5, 0.125 -> 0
    assert R.keep_mask(b, "bf16", "mxfp4", "ceil").all()
    codes, scales = R.export_bits(b, "bf16", "mxfp4", "ceil")
    assert scales.tolist() == [128] and codes[0] == 6    # 4.0 is code 6 of E2M1


@pytest.mark.parametrize("lead", [6.0, 6.5, 6.99])
def test_worked_fp4_blocks_that_round_to_six_are_unmasked(lead):
    b = block_led_by(lead, "fp32")
    assert R.keep_mask(b, "fp32", "mxfp4", "floor").all()
    assert decode(R.quantize_bits(b, "fp32", "mxfp4", "floor"), "fp32")[0, 0] == 6.0


def test_worked_mask_boundary_is_the_rounded_value():
    """|t| >= 7 rounds to 8 on the unbounded grid (masked); below 7 it rounds to 6 (kept); 7.0 itself is a tie that goes to 8 (even)"""
    for lead, kept in ((6.99, True), (7.0, False), (7.01, False), (7.9, False)):
        assert bool(R.keep_mask(block_led_by(lead, "fp32"), "fp32", "mxfp4")[0, 0]) is kept
    # E2M3: max-normal 7.5, quantum 0.5 in the top binade: below 7.75 rounds to 7.5 (kept); 7.75 is a tie between 7.5 and 8 -> 8 (even)
    for lead, kept in ((7.5, True), (7.74, True), (7.75, False), (7.9, False)):
        assert bool(R.keep_mask(block_led_by(lead, "fp32"), "fp32", "mxfp6_e2m3")[0, 0]) is kept


def test_zero_and_non_finite_blocks_are_all_ones():
    z = np.zeros((1, 32), np.uint16)
    z[0, 3] = 0x8000
    for rule in R.RULES:
        assert R.keep_mask(z, "bf16", "mxfp4", rule).all()
        assert R.export_bits(z, "bf16", "mxfp4", rule)[1].tolist() == [0]      # E = -127
        n = block_led_by(7.0).copy()
        n[0, 5] = 0x7FC0
        assert R.keep_mask(n, "bf16", "mxfp4", rule).all()
        assert R.export_bits(n, "bf16", "mxfp4", rule)[1].tolist() == [0xFF]


def test_ceil_exponent_from_subnormal_and_extreme_amax():
    sub = 2.0 ** -149 * 7                     # fp32 subnormal, mantissa 1.75: above 1.5 = 6 / 4
    assert R.shared_exp(np.array([sub]), "mxfp4", "floor").tolist() == [-127]      # -147 - 2 clamps
    assert R.shared_exp(np.array([sub]), "mxfp4", "ceil").tolist() == [-127]
    big = float(np.float32(3.4e38))
    for fmt in FMTS:
        Ef = int(R.shared_exp(np.array([big]), fmt, "floor")[0])
        Ec = int(R.shared_exp(np.array([big]), fmt, "ceil")[0])
        assert Ec in (Ef, Ef + 1) and Ec <= 127 and big * 2.0 ** -Ec <= params(fmt)[3]


# ---- the floor rule is mx_reference's; the ceil rule never saturates ------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_floor_rule_equals_mx_reference_on_every_bf16_pattern(fmt):
    b = exhaustive_bits("bf16", fmt)
    assert set(np.unique(b)) == set(range(1 << 16))
    assert np.array_equal(R.quantize_bits(b, "bf16", fmt, "floor"), M.quantize_bits(b, "bf16", fmt))
    if fmt in EXPORT_FMTS:
        got, want = R.export_bits(b, "bf16", fmt, "floor"), M.export_bits(b, "bf16", fmt)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ceil_rule_masks_nothing_on_every_pattern(fmt, dtype):
    b = exhaustive_bits(dtype, fmt)
    assert set(np.unique(b)) == set(range(1 << 16))
    leads = set(lead_bits(dtype, fmt))
    mb = int(encode(np.array([params(fmt)[3]]), dtype)[0])
    assert {mb - 1, mb, mb + 1} <= leads            # max-normal's mantissa exactly, one ulp below, one above
    assert R.keep_mask(b, dtype, fmt, "ceil").all()
    kf = R.keep_mask(b, dtype, fmt, "floor")
    assert not kf.all()                              # the same cases do saturate under floor
    # and nothing saturates in value either: |y| never exceeds the block's amax rounded up to the grid, i.e. q <= max-normal untouched
    v = decode(b, dtype).reshape(-1, 32)
    fin = np.isfinite(v).all(1)
    E = R.shared_exp(np.abs(np.where(fin[:, None], v, 0)).max(1), fmt, "ceil")
    t = np.abs(np.where(fin[:, None], v, 0)) * np.exp2(-E.astype(np.float64))[:, None]
    assert (t <= params(fmt)[3]).all()


# ---- the GPU tier's cases are sensitive: a deliberately wrong reference differs on them -----------------------------------------------

def wrong_mask(bits, dtype, fmt, rule="floor"):
    """the tempting wrong definition: masked where |t| itself, not its rounded value, exceeds max-normal"""
    v = decode(bits, dtype).reshape(-1, 32)
    fin = np.isfinite(v).all(1)
    vf = np.where(fin[:, None], v, 0.0)
    E = R.shared_exp(np.abs(vf).max(1), fmt, rule)
    t = np.abs(vf) * np.exp2(-E.astype(np.float64))[:, None]
    return (~(t > params(fmt)[3]) | ~fin[:, None]).reshape(np.asarray(bits).shape)


def gpu_value_cases(dtype, fmt):
    """what tests/test_gpu_mx_rules.py feeds the kernels for `dtype`"""
    if dtype == "fp32":
        return [rand_bits(s, "fp32", 10 + k) for k, s in enumerate([(3, 32), (257, 96), (2, 3, 4, 64)])]
    return [exhaustive_bits(dtype, fmt)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_mask_cases_catch_the_unrounded_comparison(fmt, dtype):
    n = 0
    for b in gpu_value_cases(dtype, fmt):
        n += int((wrong_mask(b, dtype, fmt) != R.keep_mask(b, dtype, fmt)).sum())
    print(f"[mask sensitivity] {fmt} {dtype}: {n} elements differ under the |t| > max-normal definition")
    assert n > 0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_ceil_cases_catch_the_floor_rule(fmt, dtype):
    ny = ns = nm = 0
    for b in gpu_value_cases(dtype, fmt):
        ny += int((R.quantize_bits(b, dtype, fmt, "ceil") != R.quantize_bits(b, dtype, fmt, "floor")).sum())
        nm += int((R.keep_mask(b, dtype, fmt, "ceil") != R.keep_mask(b, dtype, fmt, "floor")).sum())
        if fmt in EXPORT_FMTS:
            ns += int((R.export_bits(b, dtype, fmt, "ceil")[1] != R.export_bits(b, dtype, fmt, "floor")[1]).sum())
    print(f"[ceil sensitivity] {fmt} {dtype}: {ny} values, {ns} scale bytes, {nm} mask bits differ from floor")
    assert ny > 0 and nm > 0 and (ns > 0 or fmt not in EXPORT_FMTS)


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rotate", [False, True])
def test_backward_cases_catch_a_multiply_an_unmasked_and_an_unrotated_gradient(dtype, rotate):
    b = rand_bits((64, 128), dtype, 3)
    b.reshape(-1, 32)[::3, 0] = encode(np.array([7.0]), dtype)[0]       # many saturating leaders
    b.reshape(-1, 32)[::3, 1:] = encode(np.array([1.0]), dtype)[0]
    keep = R.keep_mask(b, dtype, "mxfp4", "floor", rotate)
    assert (~keep).sum() > 20
    g = grad_bits(keep, dtype, 4)
    gv = decode(g, dtype)
    assert np.isnan(gv[~keep]).any() and np.isinf(gv[~keep]).any() and np.isnan(gv[keep]).any() and np.isinf(gv[keep]).any()
    want = R.ste_backward_bits(g, keep, dtype, rotate)

    def differs(other):
        wn, on = np.isnan(decode(want, dtype)), np.isnan(decode(other, dtype))
        return not np.array_equal(wn, on) or bool(((want != other) & ~wn).any())
    with np.errstate(invalid="ignore", over="ignore"):
        mult = encode(gv * keep, dtype).reshape(g.shape)                       # NaN * 0 = NaN, -1 * 0 = -0
        assert differs(R.ste_backward_bits(mult, np.ones_like(keep), dtype, rotate))
        assert differs(R.ste_backward_bits(g, np.ones_like(keep), dtype, rotate))                  # no mask at all
        src = rotate_values(b, dtype).view(np.uint32) if rotate else b          # the unrounded comparison, on the values the quantizer sees
        wrong = wrong_mask(src, "fp32" if rotate else dtype, "mxfp4").reshape(keep.shape)
        assert (wrong != keep).any() and not wrong.all()
        assert differs(R.ste_backward_bits(g, wrong, dtype, rotate))
        assert differs(R.ste_backward_bits(g, keep, dtype, not rotate))                            # rotation forgotten / added
    if not rotate:
        assert (want[~keep] == 0).all() and np.array_equal(want[keep], g[keep])                    # +0.0 exactly; kept bits untouched


def test_rotated_mask_refers_to_the_rotated_values():
    b = rand_bits((16, 128), "bf16", 8)
    b.reshape(-1)[np.isnan(decode(b, "bf16")).reshape(-1) | np.isinf(decode(b, "bf16")).reshape(-1)] = 0
    from mx_rot_reference import rotate_values
    r = rotate_values(b, "bf16")
    assert np.array_equal(R.keep_mask(b, "bf16", "mxfp4", "floor", True), R.keep_mask(r.view(np.uint32), "fp32", "mxfp4", "floor"))
    assert np.array_equal(R.quantize_bits(b, "bf16", "mxfp4", "floor", True), __import__("mx_rot_reference").quantize_rot_bits(b, "bf16", "mxfp4"))


# ---- Python API: argument errors, defaults, attributes ------------------------------------------------------------------------------

def test_argument_errors_of_the_new_keywords():
    x = torch.zeros(4, 64)
    for call in (lambda: ops.mx_quantize(x, "mxfp4", scale_rule="round"), lambda: ops.mx_quantize(x, "mxfp4", scale_rule=None),
                 lambda: ops.mx_export(x, "mxfp4", scale_rule="up"), lambda: llm_qat_amd.mx_quantize(x, "mxfp4", scale_rule="Ceil"),
                 lambda: llm_qat_amd.mx_quantize(x, "mxfp4", ste="mask"), lambda: llm_qat_amd.mx_quantize(x, "mxfp4", ste=None),
                 lambda: MXLinear(128, 8, scale_rule="nearest")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ops.mx_quantize(x, "mxfp4", scale_rule="ceil"), lambda: ops.mx_quantize(x, "mxfp4", return_mask=True),
                 lambda: ops.mx_export(x, "mxfp4", scale_rule="ceil"), lambda: llm_qat_amd.mx_quantize(x, "mxfp4", ste="clip"),
                 lambda: ops.mx_ste_backward(x, torch.zeros(32, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="no CPU"):     # CPU tensors raise as they always did
            call()
    m8 = torch.zeros(32, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.mx_ste_backward(x, torch.zeros(31, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.mx_ste_backward(torch.zeros(4, 48), torch.zeros(24, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.mx_ste_backward(torch.zeros(4, 96), torch.zeros(48, dtype=torch.uint8), rotate=True)
    with pytest.raises(TypeError):
        ops.mx_ste_backward(x, m8.int())
    with pytest.raises(TypeError):
        ops.mx_ste_backward(x, None)
    with pytest.raises(ValueError):
        ops.mx_export(x, "mxfp6_e2m3", scale_rule="ceil")


def test_process_defaults_return_the_previous_value_and_reach_new_layers():
    assert llm_qat_amd.default_mx_scale_rule("ceil") == "floor"
    try:
        assert llm_qat_amd.default_mx_ste("clip") == "identity"
        try:
            m = QuantizeLinear(64, 32, w_bits=4, a_bits=8, weight_format="mxfp4")
            assert m.mx_scale_rule == "ceil" and m.mx_ste == "clip"
            plain = QuantizeLinear(64, 32, w_bits=4, a_bits=8)                     # no MX operand: untouched
            assert plain.mx_scale_rule == "floor" and plain.mx_ste == "identity"
            e = QuantizeLinear(64, 32, w_bits=4, a_bits=8, act_format="mxfp8_e4m3", mx_scale_rule="floor", mx_ste="identity")
            assert e.mx_scale_rule == "floor" and e.mx_ste == "identity"          # explicit wins
        finally:
            assert llm_qat_amd.default_mx_ste("identity") == "clip"
    finally:
        assert llm_qat_amd.default_mx_scale_rule("floor") == "ceil"
    for bad in ("", "CEIL", None, 1):
        with pytest.raises(ValueError):
            llm_qat_amd.default_mx_scale_rule(bad)
        with pytest.raises(ValueError):
            llm_qat_amd.default_mx_ste(bad)
    assert llm_qat_amd.default_mx_scale_rule("floor") == "floor" and llm_qat_amd.default_mx_ste("identity") == "identity"


def test_quantize_linear_keywords():
    m = QuantizeLinear(128, 32, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_scale_rule="ceil", mx_ste="clip")
    assert m.mx_scale_rule == "ceil" and m.mx_ste == "clip"
    ref = QuantizeLinear(128, 32, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3")
    assert ref.mx_scale_rule == "floor" and ref.mx_ste == "identity"
    assert set(m.state_dict()) == set(ref.state_dict()) == {"weight"}
    for kw in ({"mx_scale_rule": "ceil"}, {"mx_ste": "clip"}, {"mx_scale_rule": "floor"}, {"mx_ste": "identity"}):
        with pytest.raises(ValueError, match="MX operand"):
            QuantizeLinear(128, 32, w_bits=4, a_bits=8, **kw)
    with pytest.raises(ValueError):
        QuantizeLinear(128, 32, weight_format="mxfp4", mx_scale_rule="up")
    with pytest.raises(ValueError):
        QuantizeLinear(128, 32, weight_format="mxfp4", mx_ste="mask")
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(2, 128))
    with pytest.raises(RuntimeError, match="no CPU"):
        m.export_weight()


def test_mxlinear_carries_the_rule():
    m = MXLinear(128, 16, scale_rule="ceil")
    assert m.scale_rule == "ceil" and "scale_rule='ceil'" in repr(m)
    d = MXLinear(128, 16)
    assert d.scale_rule == "floor" and "scale_rule" not in repr(d)
    assert set(m.state_dict()) == set(d.state_dict())


def test_signatures_of_the_public_functions():
    def names(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert names(ops.mx_quantize) == [("x", inspect._empty), ("fmt", inspect._empty), ("rotate", False), ("scale_rule", "floor"), ("return_mask", False)]
    assert names(ops.mx_export) == [("x", inspect._empty), ("fmt", inspect._empty), ("rotate", False), ("scale_rule", "floor")]
    assert names(ops.mx_ste_backward) == [("g", inspect._empty), ("mask", inspect._empty), ("rotate", False)]
    assert names(llm_qat_amd.mx_quantize) == [("x", inspect._empty), ("fmt", inspect._empty), ("rotate", False), ("scale_rule", "floor"), ("ste", "identity")]
    assert list(inspect.signature(llm_qat_amd.default_mx_scale_rule).parameters) == ["rule"]
    assert list(inspect.signature(llm_qat_amd.default_mx_ste).parameters) == ["mode"]
    assert list(inspect.signature(llm_qat_amd.default_mx_formats).parameters) == ["weight", "act"]          # pinned, unchanged
    p = inspect.signature(QuantizeLinear.__init__).parameters
    assert p["mx_scale_rule"].default is None and p["mx_ste"].default is None
    p = inspect.signature(MXLinear.__init__).parameters
    assert p["scale_rule"].default == "floor" and p["rotate"].default is False
    for name in ("default_mx_scale_rule", "default_mx_ste"):
        assert name in llm_qat_amd.__all__
    for k in ("mx_mask_launch", "mx_ste_launch"):
        assert k in ops.mx_counts
    from llm_qat_amd import compiled
    for op in ("mx_fake_quant_rule", "mx_fake_quant_clip", "mx_ste_backward", "mx_export_rule", "mx_fake_quant", "mx_fake_quant_rot", "mx_export"):
        assert hasattr(torch.ops.llmqat_amd, op)
    assert str(compiled.mx_fake_quant_op._opoverload._schema) == "llmqat_amd::mx_fake_quant(Tensor x, str fmt) -> Tensor"     # existing schemas stay


# ---- C ABI: header, EXPORTS and validation codes (no launch) ------------------------------------------------------------------------------

NEW = {"fq_mx_fwd_ex": "pppqqiiip", "fq_mx_export_ex": "pppqqiiip", "fq_mx_ste_bwd": "pppqqiip"}


def test_header_declares_the_new_entry_points_and_exports_agree():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "llmqat_fakequant.h")).read()
    assert re.search(r"^#define FQ_ABI_VERSION 7\b", hdr, re.M)
    assert re.search(r"^#define FQ_MX_FLAG_ROTATE 1$", hdr, re.M) and re.search(r"^#define FQ_MX_FLAG_CEIL 2$", hdr, re.M)
    assert (_lib.MX_FLAG_ROTATE, _lib.MX_FLAG_CEIL) == (1, 2)
    L = _lib.lib()
    for name, kinds in NEW.items():
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, re.M | re.S)
        assert m, f"{name} is not declared"
        args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        got = "".join("p" if "*" in a else "q" if a.startswith("int64_t") else "i" for a in args)
        assert got == kinds
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert "".join("p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64 else "i" for t in fn.argtypes) == kinds
    # the seven-argument entry points keep their signatures
    for name, kinds in (("fq_mx_fwd", "ppqqiip"), ("fq_mx_export", "pppqqiip"), ("fq_mx_fwd_rot", "ppqqiip"), ("fq_mx_export_rot", "pppqqiip")):
        fn = getattr(L, name)
        assert "".join("p" if t is ctypes.c_void_p else "q" if t is ctypes.c_int64 else "i" for t in fn.argtypes) == kinds


def test_abi_validation_codes_of_the_new_entry_points():
    L = _lib.lib()
    assert L.fq_version() == 7
    fake = 1 << 20        # a 16-byte-aligned non-NULL address: never dereferenced, validation fails first
    a, b, c = fake, fake + 4096, fake + 8192
    BF, F16, F32, F64 = _lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32, _lib.DTYPE_F64
    fwd, exp, bwd = L.fq_mx_fwd_ex, L.fq_mx_export_ex, L.fq_mx_ste_bwd
    for flags in (0, 1, 2, 3):
        assert fwd(a, b, c, 4, 64, 0, F64, flags, None) == -1
        assert fwd(a, b, c, 4, 64, 0, 9, flags, None) == -1
        assert fwd(a, b, c, 4, 64, 5, BF, flags, None) == -7
        assert fwd(a, b, c, 4, 64, -1, BF, flags, None) == -7
        assert fwd(a, a, c, 4, 64, 0, BF, flags, None) == -7                  # y == x
        assert fwd(a, b, c, 4, 48, 0, BF, flags, None) == -3
        assert fwd(a, b, c, -1, 64, 0, BF, flags, None) == -3
        assert fwd(None, b, c, 4, 64, 0, BF, flags, None) == -4
        assert fwd(a, None, c, 4, 64, 0, BF, flags, None) == -4
        assert fwd(a + 2, b, c, 4, 64, 0, BF, flags, None) == -8
        assert fwd(a, b + 8, c, 4, 64, 0, F32, flags, None) == -8
        assert fwd(a, b, c + 4, 4, 64, 0, F16, flags, None) == -8               # the mask is 16-byte aligned too
        assert fwd(None, None, None, 0, 64, 0, BF, flags, None) == 0            # empty: no launch
        assert fwd(None, None, None, 5, 0, 2, F16, flags, None) == 0
        assert exp(a, b, c, 4, 64, 1, BF, flags, None) == -7                    # FP6 export
        assert exp(a, b, c, 4, 64, 2, F32, flags, None) == -7
        assert exp(a, b, c, 4, 64, 7, F32, flags, None) == -7
        assert exp(a, b, c, 4, 64, 0, F64, flags, None) == -1
        assert exp(a, b, c, 4, 48, 3, F16, flags, None) == -3
        assert exp(a, None, c, 4, 64, 3, F16, flags, None) == -4
        assert exp(a, b, None, 4, 64, 3, F16, flags, None) == -4
        assert exp(None, b, c, 4, 64, 3, F16, flags, None) == -4
        assert exp(a, b, c + 8, 4, 64, 3, F16, flags, None) == -8
        assert exp(a, b + 4, c, 4, 64, 0, F16, flags, None) == -8
        assert exp(None, None, None, 7, 0, 4, F32, flags, None) == 0
    for flags in (0, 1, 2, 3):                                                    # the bitmap may not be x or y, nor g or gx
        assert fwd(a, b, a, 4, 64, 0, BF, flags, None) == -7 and fwd(a, b, b, 4, 64, 0, BF, flags, None) == -7
    assert bwd(a, a, c, 4, 64, BF, 0, None) == -7 and bwd(a, c, c, 4, 64, BF, 1, None) == -7
    assert fwd(a, b, c, 4, 96, 0, BF, 1, None) == -3 and fwd(a, b, c, 4, 96, 0, BF, 3, None) == -3      # rotate: a multiple of 64
    assert exp(a, b, c, 4, 96, 0, BF, 1, None) == -3
    for flags in (4, 8, 7, -1, 1 << 30):                                          # unknown flag bits
        assert fwd(a, b, c, 4, 64, 0, BF, flags, None) == -7
        assert exp(a, b, c, 4, 64, 0, BF, flags, None) == -7
        assert bwd(a, b, c, 4, 64, BF, flags, None) == -7
    assert bwd(a, b, c, 4, 64, BF, 2, None) == -7                                 # the backward has no scale rule
    for flags in (0, 1):
        assert bwd(a, b, c, 4, 64, F64, flags, None) == -1
        assert bwd(a, b, c, 4, 64, -1, flags, None) == -1
        assert bwd(a, b, c, 4, 48, BF, flags, None) == -3
        assert bwd(a, b, c, -4, 64, BF, flags, None) == -3
        assert bwd(a, b, c, 2 ** 62, 64, BF, flags, None) == -3
        assert bwd(None, b, c, 4, 64, BF, flags, None) == -4
        assert bwd(a, None, c, 4, 64, BF, flags, None) == -4
        assert bwd(a, b, None, 4, 64, BF, flags, None) == -4
        assert bwd(a + 2, b, c, 4, 64, BF, flags, None) == -8
        assert bwd(a, b + 4, c, 4, 64, BF, flags, None) == -8
        assert bwd(a, b, c + 8, 4, 64, F32, flags, None) == -8
        assert bwd(None, None, None, 0, 64, BF, flags, None) == 0
        assert bwd(None, None, None, 3, 0, F32, flags, None) == 0
    assert bwd(a, b, c, 4, 96, BF, 1, None) == -3
    assert bwd(a, b, a, 4, 64, BF, 1, None) == -7                                 # in place: refused with the rotation ...
    assert b"in-place" in L.fq_last_error()
    # ... and served without it (tests/test_gpu_mx_rules.py runs it; a launch on made-up addresses is not for this tier)


def test_abi_fuzz_covers_the_new_names():
    import test_abi_and_host as T
    T.test_library_exports_every_declared_symbol()
    T.test_abi_rejects_null_pointers_and_hostile_sizes_before_any_launch()
