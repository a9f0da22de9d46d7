"""The MX block-scaled GEMM (fq_mx_gemm / ops.mx_matmul / MXLinear) on the MI355X against the float64 reference of
tests/mx_gemm_reference.py.  Exact tier (zero tolerance: inputs whose every partial sum is an fp32 value, so any summation order gives the
same bits): operand layout with one-hot rows, exact sums on both launch shapes, run-to-run identity, the NaN rule, canaries.  Bounded
tier: Gaussian tensors through ops.mx_export under the any-order fp32 accumulation bound |out - ref| <= 2 * K * 2^-24 * sum_k |a w|."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import llm_qat_amd
from llm_qat_amd import MXLinear, _lib, convert_to_mx_inference, ops
from llm_qat_amd.utils_quant import QuantizeLinear

from mx_gemm_reference import GEMM_FMTS, PAIRS, export_from_codes, grid_operand, prove_exact, ref64, to_cpu, to_device

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def run(a, w, out_dtype=torch.float32):
    return ops.mx_matmul(to_device(a), to_device(w), out_dtype=out_dtype).cpu()


def assert_exact(out, ref):
    want = ref.to(torch.float32)
    assert want.double().equal(ref), "the reference itself is not an fp32 value"
    bad = torch.nonzero(out.view(torch.int32).reshape(want.shape) != want.view(torch.int32))
    assert bad.numel() == 0, f"{bad.shape[0]} of {want.numel()} differ, first at {bad[:4].tolist()}: got {out.reshape(want.shape)[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _asym_codes(rows, K, fmt, salt):
    """codes distinct along rows and k (nonzero finite values of both signs) and scales that differ from block to block and row to row"""
    r, k = np.arange(rows)[:, None], np.arange(K)[None, :]
    if fmt == "mxfp4":
        codes = (r * 3 + k * 5 + salt) % 7 + 1 + 8 * ((r + k // 3) % 2)
    else:
        codes = (r * 37 + k * 11 + salt) % 100 + 8 + 128 * ((r + k // 3) % 2)    # 8 .. 107: normal, below every special code
    scales = 120 + (r * 5 + (k[:, ::32] // 32) * 3 + salt) % 13
    return codes.astype(np.uint8), scales.astype(np.uint8)


def _one_hot(rows, K, fmt, salt):
    """row i: a single 1.5 at k = i % K, code 0 elsewhere; scales differ per block and row"""
    codes = np.zeros((rows, K), dtype=np.uint8)
    codes[np.arange(rows), np.arange(rows) % K] = {"mxfp4": 0x3, "mxfp8_e4m3": 0x3C, "mxfp8_e5m2": 0x3E}[fmt]
    r, kb = np.arange(rows)[:, None], np.arange(K // 32)[None, :]
    return codes, (118 + (r * 7 + kb * 5 + salt) % 17).astype(np.uint8)


@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_layout_one_hot_sweeps_k_over_both_operands(a_fmt, w_fmt):
    """k = 0 .. 255 (two K steps of the kernel) as the single nonzero of a row of A against an asymmetric W, then of a row of W against an
    asymmetric A; per-block, per-row scales on both.  A wrong nibble, byte, lane or scale assignment changes a value."""
    K = 256
    hot_a = export_from_codes(*_one_hot(256, K, a_fmt, 1), a_fmt)
    asym_w = export_from_codes(*_asym_codes(40, K, w_fmt, 2), w_fmt)
    ref, _ = ref64(hot_a, asym_w)
    assert_exact(run(hot_a, asym_w), ref)                                   # tiled route, M = 256
    for m0 in range(0, 256, 32):                                           # skinny route, 32 rows at a time
        sub = export_from_codes(_one_hot(256, K, a_fmt, 1)[0][m0:m0 + 32], _one_hot(256, K, a_fmt, 1)[1][m0:m0 + 32], a_fmt)
        assert_exact(run(sub, asym_w), ref[m0:m0 + 32])
    hot_w = export_from_codes(*_one_hot(256, K, w_fmt, 3), w_fmt)
    for M in (40, 23):                                                      # tiled, skinny
        asym_a = export_from_codes(*_asym_codes(M, K, a_fmt, 4), a_fmt)
        assert_exact(run(asym_a, hot_w), ref64(asym_a, hot_w)[0])


def _exact_case(M, N, K, a_fmt, w_fmt, seed):
    rng = np.random.default_rng(seed)
    a, ai = grid_operand(rng, M, K, a_fmt)
    w, wi = grid_operand(rng, N, K, w_fmt)
    prove_exact(ai, wi)
    return a, w


@pytest.mark.parametrize("M,N,K,a_fmt,w_fmt", [(2048, 11008, 4096, "mxfp8_e4m3", "mxfp4"), (2048, 4096, 11008, "mxfp8_e4m3", "mxfp4")])
def test_exact_sums_llama_shapes(M, N, K, a_fmt, w_fmt):
    a, w = _exact_case(M, N, K, a_fmt, w_fmt, 11)
    llm_qat_amd.stats(reset=True)
    out = run(a, w)
    st = llm_qat_amd.stats()
    assert st.get("mx_gemm_tiled") == 1 and st.get("mx_gemm_launch") == 1 and "mx_gemm_skinny" not in st
    assert_exact(out, ref64(a, w)[0])


@pytest.mark.parametrize("N", [1, 100, 4096])
@pytest.mark.parametrize("M", [1, 7, 16, 32, 33, 129])
def test_exact_sums_edge_shapes(M, N):
    K = 4096
    a_fmt, w_fmt = PAIRS[(M + N) % 9]
    a, w = _exact_case(M, N, K, a_fmt, w_fmt, 100 * M + N)
    llm_qat_amd.stats(reset=True)
    out = run(a, w)
    st = llm_qat_amd.stats()
    assert st.get("mx_gemm_skinny" if M <= 32 else "mx_gemm_tiled") == 1 and st.get("mx_gemm_launch") == 1
    assert_exact(out, ref64(a, w)[0])


@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_exact_sums_every_pair_both_routes(a_fmt, w_fmt):
    for M, N, K in ((16, 208, 1408), (200, 136, 1408)):   # K = 11 steps: odd, not a multiple of the skinny kernel's 8-wave split
        a, w = _exact_case(M, N, K, a_fmt, w_fmt, M)
        assert_exact(run(a, w), ref64(a, w)[0])


@pytest.mark.parametrize("M", [16, 2048])
def test_run_to_run_identical(M):
    x = torch.randn(M, 4096, device="cuda", dtype=torch.bfloat16)
    wt = torch.randn(1000, 4096, device="cuda", dtype=torch.bfloat16)
    a, w = ops.mx_export(x, "mxfp8_e4m3"), ops.mx_export(wt, "mxfp4")
    o1 = ops.mx_matmul(a, w, out_dtype=torch.float32)
    o2 = ops.mx_matmul(a, w, out_dtype=torch.float32)
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32))


@pytest.mark.parametrize("M", [20, 150])
@pytest.mark.parametrize("a_fmt,w_fmt", [("mxfp8_e4m3", "mxfp4"), ("mxfp4", "mxfp8_e5m2")])
def test_nan_scale_block_poisons_exactly_its_row_or_column(M, a_fmt, w_fmt):
    N, K = 150, 512
    a, w = _exact_case(M, N, K, a_fmt, w_fmt, 5)
    base = run(a, w)
    assert not torch.isnan(base).any()
    a2 = to_cpu(a)
    a2.scales = a.scales.clone()
    a2.scales[M - 3, 9] = 0xFF
    out = run(a2, w)
    assert torch.isnan(out[M - 3]).all()
    keep = torch.ones(M, dtype=torch.bool)
    keep[M - 3] = False
    assert torch.equal(out[keep], base[keep])
    w2 = to_cpu(w)
    w2.scales = w.scales.clone()
    w2.scales[77, 0] = 0xFF
    out = run(a, w2)
    assert torch.isnan(out[:, 77]).all()
    keep = torch.ones(N, dtype=torch.bool)
    keep[77] = False
    assert torch.equal(out[:, keep], base[:, keep])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N", [(130, 100), (130, 333), (31, 333), (5, 7), (257, 130)])
def test_canaries_around_out_with_tails(M, N, dtype):
    """the raw entry point writes out[M, N] and nothing else: tails in M and N (N % 4 != 0 takes the element-wise stores)"""
    K = 256
    a, w = _exact_case(M, N, K, "mxfp8_e4m3", "mxfp4", 9)
    ad, wd = to_device(a), to_device(w)
    pad = 4096
    es = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((pad + M * N * es + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    code = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}[dtype]
    rc = L.fq_mx_gemm(ad.elements.data_ptr(), ad.scales.data_ptr(), ops.MX_FORMATS[a.fmt], wd.elements.data_ptr(), wd.scales.data_ptr(),
                      ops.MX_FORMATS[w.fmt], buf.data_ptr() + pad, M, N, K, code, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.fq_last_error()
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:pad] == 0xA5).all() and (host[pad + M * N * es:] == 0xA5).all()
    out = host[pad:pad + M * N * es].view(dtype).reshape(M, N)
    ref = ref64(a, w)[0]
    assert torch.equal(out.double(), ref.to(dtype).double())   # exact sums: the one rounding to the output dtype is the reference's


# ---- bounded tier -----------------------------------------------------------------------------------------------------------------------
def _bounded(out, ref, S, K, what):
    ratio = ((out.double() - ref).abs() / (U * S).clamp_min(1e-300)).max().item()
    print(f"[mx_gemm accumulation error] {what}: max |out - ref| / (2^-24 S) = {ratio:.4f}  (bound {2 * K})")
    assert ratio <= 2 * K, f"{what}: {ratio} > 2K = {2 * K}"
    return ratio


def _check_rounded(out, ref, S, K, dtype, out32=None):
    """A 16-bit output against the float64 reference under the fp32 bound b = 2 K 2^-24 S: the kernel rounds its fp32 sum once, the sum
    lies in [ref - b, ref + b], and rounding is monotone, so out lies in [RN(ref - b), RN(ref + b)].  Where the bound cannot move the sum
    across a rounding boundary the two ends coincide and out must equal the correctly rounded reference; where it spans one boundary they
    are the two neighbouring values.  For these tensors b (about 0.06 at K = 4096, S about 125) exceeds the bf16 spacing of most outputs,
    so the interval usually spans several values; the literal "one of the two values next to the reference" is then not implied by the
    fp32 bound and is not met: measured on MI355X, up to 66 of 6144 and 562 of 61440 outputs per case (fp16, the finer spacing, the most),
    and 8430 of 22.5 M / 3186 of 8.4 M bf16 outputs of MXLinear at 4096 -> 11008 / 11008 -> 4096, lie further from the reference than one
    spacing of the dtype: outputs near zero (cancellation; largest |ref| among them 0.33, at the LLaMA shapes 0.006) whose 16-bit spacing
    is finer than the fp32 sum's own rounding error (measured: up to 28.6 * 2^-24 S, S about 125 .. 340).  The count is printed.
    out32 (the fp32 output of the same operands) pins the 16-bit result completely: it must be RN(out32), bit for bit."""
    b = 2 * K * U * S
    lo, hi = (ref - b).to(dtype), (ref + b).to(dtype)
    r = ref.to(dtype)
    settled = lo == hi
    step = torch.finfo(dtype).eps * ref.abs()                      # at least the spacing of dtype at ref
    beyond = (out.double() - ref).abs() > step
    print(f"[mx_gemm {dtype}] {int((~settled).sum())} of {out.numel()} outputs within the fp32 bound of a rounding boundary; "
          f"{int(beyond.sum())} further from the reference than its two neighbours (max |ref| among them {ref[beyond].abs().max().item() if beyond.any() else 0:.3g})")
    assert (out[settled] == r[settled]).all()
    ok = (out.double() >= lo.double()) & (out.double() <= hi.double())
    assert ok.all(), f"{(~ok).sum().item()} of {ok.numel()} {dtype} outputs lie outside [RN(ref - b), RN(ref + b)]"
    if out32 is not None:
        assert torch.equal(out.view(torch.int16), out32.to(dtype).view(torch.int16)), "the 16-bit output is not the one rounding of the fp32 sum"


@pytest.mark.parametrize("K", [4096, 11008])
@pytest.mark.parametrize("a_fmt,w_fmt", PAIRS)
def test_gaussian_within_the_fp32_accumulation_bound(a_fmt, w_fmt, K):
    g = torch.Generator(device="cuda").manual_seed(K)
    for M, N in ((16, 384), (160, 384)):
        x = torch.randn(M, K, device="cuda", generator=g)
        wt = torch.randn(N, K, device="cuda", generator=g) * 0.05
        a, w = ops.mx_export(x, a_fmt), ops.mx_export(wt, w_fmt)
        ref, S = ref64(to_cpu(a), to_cpu(w))
        out = ops.mx_matmul(a, w, out_dtype=torch.float32).cpu()
        _bounded(out, ref, S, K, f"A {a_fmt} x W {w_fmt} K={K} M={M}")
        for dtype in (torch.bfloat16, torch.float16):
            _check_rounded(ops.mx_matmul(a, w, out_dtype=dtype).cpu(), ref, S, K, dtype, out32=out)


def _layer(i, o, wf="mxfp4", af="mxfp8_e4m3", seed=0):
    torch.manual_seed(seed)
    layer = QuantizeLinear(i, o, w_bits=4, a_bits=8, weight_format=wf, act_format=af).to("cuda", torch.bfloat16)
    with torch.no_grad():
        layer.weight.normal_(0, 0.02)
    return layer.eval()


def _layer_reference(layer, x):
    a = to_cpu(ops.mx_export(x, layer.act_format))
    w = to_cpu(ops.mx_export(layer.weight.detach(), layer.weight_format))
    return ref64(a, w)


def _check_mx_linear(mxl, layer, x):
    ref, S = _layer_reference(layer, x)
    K = layer.in_features
    llm_qat_amd.stats(reset=True)
    with torch.no_grad():
        y = mxl(x)
    st = llm_qat_amd.stats()
    assert st.get("mx_export_launch") == 1 and st.get("mx_gemm_launch") == 1 and "mx_launch" not in st   # 2 launches per call
    assert y.dtype == x.dtype and y.shape == x.shape[:-1] + (layer.out_features,)
    a = ops.mx_export(x, layer.act_format)
    out32 = ops.mx_matmul(a, ops.mx_export(layer.weight.detach(), layer.weight_format), out_dtype=torch.float32).cpu().reshape(ref.shape)
    _bounded(out32, ref, S, K, f"MXLinear {K}->{layer.out_features}")
    _check_rounded(y.cpu().reshape(ref.shape), ref, S, K, x.dtype, out32=out32)
    return ref, S


@pytest.mark.parametrize("i,o", [(4096, 11008), (11008, 4096)])
def test_mx_linear_against_the_float64_reference_llama_shapes(i, o):
    layer = _layer(i, o)
    x = torch.randn(2048, i, device="cuda", dtype=torch.bfloat16)
    mxl = MXLinear.from_quantize_linear(layer)
    assert not any(p.dtype == torch.bfloat16 and p.numel() >= i * o for p in list(mxl.parameters()) + list(mxl.buffers()))
    ref, S = _check_mx_linear(mxl, layer, x)
    # the eval-mode QuantizeLinear (fake quant + bf16 library GEMM) against the same reference, with its own bound: its operands are the
    # dequantized values exactly (FP4 / E4M3 values times a power of two are bf16 values), its products are exact in fp32, its fp32
    # accumulation in any order errs by at most K * 2^-24 * S (doubled, as for the kernel, for a truncating adder), and the result is
    # rounded once to bf16: half an ulp, 2^-9 relative, of a value within that bound of the reference
    with torch.no_grad():
        yq = layer(x).cpu().double()
    b = 2 * i * U * S
    assert ((yq - ref).abs() <= b + 2.0 ** -9 * (ref.abs() + b)).all()


def test_mx_linear_refuses_a_gradient():
    layer = _layer(256, 64)
    mxl = MXLinear.from_quantize_linear(layer)
    x = torch.randn(4, 256, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        mxl(x)
    with torch.no_grad():
        assert mxl(x).shape == (4, 64)


class _Stack(nn.Module):
    def __init__(self):
        super().__init__()
        self.up = QuantizeLinear(256, 768, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3")
        self.mid = QuantizeLinear(768, 768, w_bits=4, a_bits=8, weight_format="mxfp8_e4m3", act_format="mxfp8_e5m2")
        self.int8 = QuantizeLinear(768, 256, w_bits=8, a_bits=8)
        self.down = QuantizeLinear(256, 256, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp4")
        self.head = nn.Linear(256, 32, bias=False)

    def forward(self, x):
        return self.head(self.down(self.int8(self.mid(self.up(x)))))


def test_convert_to_mx_inference_swaps_exactly_the_mx_layers():
    torch.manual_seed(3)
    model = _Stack().to("cuda", torch.bfloat16).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    before = {n: copy.deepcopy(getattr(model, n)) for n in ("up", "mid", "down")}
    int8, head = model.int8, model.head
    second = copy.deepcopy(model)
    assert convert_to_mx_inference(model) == 3
    assert all(isinstance(getattr(model, n), MXLinear) for n in ("up", "mid", "down"))
    assert model.int8 is int8 and model.head is head
    x = torch.randn(64, 256, device="cuda", dtype=torch.bfloat16)
    for n, xin in (("up", x), ("mid", torch.randn(64, 768, device="cuda", dtype=torch.bfloat16)), ("down", x)):
        _check_mx_linear(getattr(model, n), before[n], xin)
    with torch.no_grad():
        for p in second.parameters():          # a second copy with other weights: the state dict must carry everything
            p.normal_(0, 0.02)
        assert convert_to_mx_inference(second) == 3
        y1 = model(x)
        assert not torch.equal(second(x), y1)
        second.load_state_dict(model.state_dict())
        assert torch.equal(second(x).view(torch.int16), y1.view(torch.int16))


@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_mx_linear_compiles_fullgraph(backend):
    layer = _layer(512, 384)
    mxl = MXLinear.from_quantize_linear(layer)
    x = torch.randn(48, 512, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        eager = mxl(x)
        got = torch.compile(mxl, fullgraph=True, backend=backend)(x)
    assert torch.equal(got.view(torch.int16), eager.view(torch.int16))
