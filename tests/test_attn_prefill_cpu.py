"""CPU tier of the fused prefill attention: every refusal of fqp_attn_prefill_fwd through ctypes and their order,
the opt-in CPU route against the float64 reference, fake tensors through the compiled op, install / convert with and without prefill."""
import ctypes
import os
import re

import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, attention, compiled, ops

import attn_prefill_reference as R
from conftest import ROOT
from test_attn_softmax_cpu import _stub_namespace

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 14))
Q, K, V, M, OUT = (P0 + 2048 * i for i in range(5))
OK = dict(q=Q, k=K, v=V, m=M, out=OUT, qs=(4096, 128, 256), ks=(4096, 128, 256), vs=(4096, 128, 256), mbs=0, mrs=4096, B=1, H=2, T=200,
          S=4096, D=64, inv=0.125, ds=1, dm=0, causal=0)
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
REFUSALS = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=3), DTYPE, "not served"), (dict(ds=0), DTYPE, "not served"), (dict(dm=7), DTYPE, "unknown"),
    (dict(ds=1, dm=2), DTYPE, "pair"), (dict(T=0), SHAPE, "positive"), (dict(D=96), SHAPE, "head size"), (dict(B=0), SHAPE, "positive"),
    (dict(S=-1), SHAPE, "positive"), (dict(qs=(4096, -128, 256)), SHAPE, "negative stride"), (dict(mrs=-1), SHAPE, "negative mask stride"),
    (dict(B=2 ** 40, H=2 ** 40), SHAPE, "overflows"), (dict(ks=(2 ** 61, 128, 256), B=4), SHAPE, "overflows"),
    (dict(m=None, causal=1, T=4097), SHAPE, "causal"), (dict(q=None), NULL, "NULL"), (dict(out=None), NULL, "NULL"), (dict(out=K), ARG, "in-place"),
    (dict(out=M), ARG, "in-place"), (dict(causal=1), ARG, "causal together with a mask"),
    (dict(B=2 ** 10, H=2 ** 7, T=1, S=1, ks=(0, 0, 0), qs=(0, 0, 0), vs=(0, 0, 0)), UNSUPPORTED, "grid"),
    # the header's order, one fault of each later class behind the first; no mask: neither its dtype code nor its strides are looked at
    (dict(ds=3, T=0, q=None, out=K, B=2 ** 17), DTYPE, ""), (dict(T=0, q=None, out=K, B=2 ** 17), SHAPE, ""), (dict(q=None, out=K, B=2 ** 17), NULL, ""),
    (dict(out=K, B=2 ** 17), ARG, ""), (dict(m=None, dm=9, mrs=-1, B=2 ** 17), UNSUPPORTED, ""),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(kw, code, text):
    a, L = dict(OK, **kw), _lib.lib()
    rc = L.fqp_attn_prefill_fwd(a["q"], a["k"], a["v"], a["m"], a["out"], *a["qs"], *a["ks"], *a["vs"], a["mbs"], a["mrs"],
                                a["B"], a["H"], a["T"], a["S"], a["D"], a["inv"], a["ds"], a["dm"], a["causal"], None)
    assert rc == code and text in L.fq_last_error().decode(), (rc, L.fq_last_error())


def test_the_header_declares_the_exports():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_prefill.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fqp_[a-z0-9_]+)\s*\(", src)) == set(_lib.PREFILL_EXPORTS) and _lib.lib().fq_version() == 7


@pytest.fixture
def cpu_route():
    llm_qat_amd.allow_cpu_tensors(True)
    yield
    llm_qat_amd.allow_cpu_tensors(False)


@pytest.mark.parametrize("dtype,kind", [(torch.bfloat16, "f32"), (torch.float16, "ds"), (torch.bfloat16, "none"), (torch.float16, "causal")])
def test_the_cpu_route_is_the_float64_chain_within_one_output_rounding(dtype, kind, cpu_route):
    """one rounding of the output is at most u |out| <= u sum p |v|: C_out <= 1, and 2^-10 for the route's fp32 softmax (2^-21 of u)"""
    T, S, D = 37, 77, 64                                                    # sqrt(64) = 8: the CPU's division is the device's product
    q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, "cpu")
    out = attention.prefill_attention(q, k, v, mask, D, causal=causal)
    assert out.shape == (R.B, R.H, T, D) and out.transpose(1, 2).is_contiguous()
    assert R.c_out(out, *R.ref64(q, k, v, ref_mask, R.inv_of(D))) <= 1 + 2.0 ** -10
    llm_qat_amd.allow_cpu_tensors(False)
    for bad, exc, text in ((dict(), RuntimeError, "allow_cpu_tensors"), (dict(q=q.clone().requires_grad_(True)), RuntimeError, "forward only"),
                           (dict(mask=torch.zeros(R.B, 1, T, S), causal=True), ValueError, "causal"), (dict(k=k[:, :, :5], v=v[:, :, :5], causal=True), ValueError, "T <= S"),
                           (dict(causal=1), TypeError, "bool"), (dict(q=q.float()), TypeError, None), (dict(q=q[..., :32]), ValueError, None)):
        a = dict(dict(q=q, k=k, v=v, mask=None, causal=False), **bad)
        with pytest.raises(exc, match=text):
            attention.prefill_attention(a["q"], a["k"], a["v"], a["mask"], D, causal=a["causal"])


def test_fake_tensors_through_the_compiled_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, k = (torch.empty(2, n, 3 * 128, dtype=torch.float16, device="cuda").view(2, n, 3, 128).transpose(1, 2) for n in (400, 900))
        out = compiled.attn_prefill_op(q, k, k, torch.empty(2, 1, 400, 900, device="cuda"), 0.1, False)
        assert out.shape == (2, 400, 3, 128) and out.dtype == torch.float16 and out.is_contiguous()
        with pytest.raises(ValueError):
            compiled.attn_prefill_op(k, q, q, None, 0.1, True)


def test_install_and_convert_take_prefill_and_leave_the_defaults_as_they_were(cpu_route):
    ns = _stub_namespace()
    parent = ns.LlamaAttention
    assert attention.install(ns) is parent and ns.LlamaAttention.fused_attn_prefill is False and ns.LlamaAttention.fused_attn_decode is False
    ns.LlamaAttention = parent
    attention.install(ns, prefill=True)
    assert ns.LlamaAttention.fused_attn_prefill is True and ns.LlamaAttention.fused_attn_decode is False and issubclass(ns.LlamaAttention, parent)
    a, b, c = (torch.nn.ModuleList([parent()]) for _ in range(3))
    assert attention.convert(a) == 1 and attention.convert(b, prefill=True) == 1 and attention.convert(c, decode=True, prefill=True) == 1
    assert len({type(a[0]), type(b[0]), type(c[0])}) == 3 and not a[0].fused_attn_prefill and b[0].fused_attn_prefill and not b[0].fused_attn_decode
    h, pos = torch.randn(1, 2, 32), torch.arange(2)[None]                   # CPU tensors are not the device's: counted fallbacks, the three calls
    for m, dec, pre in ((a[0], 0, 0), (b[0], 0, 1), (c[0], 1, 1)):
        before = dict(ops.decode_counts), dict(ops.prefill_counts)
        m.load_state_dict(a[0].state_dict())
        assert torch.equal(a[0](h, position_ids=pos)[0], m(h, position_ids=pos)[0])
        assert ops.decode_counts == dict(before[0], fallback=before[0]["fallback"] + dec)
        assert ops.prefill_counts == dict(before[1], fallback=before[1]["fallback"] + pre)
    assert attention.__all__ == ["attn_softmax", "install", "convert"]
