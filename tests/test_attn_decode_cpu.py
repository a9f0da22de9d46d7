"""CPU tier of the fused decode attention: every refusal of the fqd_ entry points through ctypes and their order,
the opt-in CPU route against the float64 reference, fake tensors through the compiled op, install / convert with and without decode."""
import ctypes
import os
import re

import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, attention, compiled, ops

import attn_decode_reference as R
from conftest import ROOT
from test_attn_softmax_cpu import _stub_namespace

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 14))
Q, K, V, M, OUT, WS = (P0 + 2048 * i for i in range(6))
OK = dict(q=Q, k=K, v=V, m=M, out=OUT, ws=WS, wsb=1 << 30, qs=(4096, 128, 256), ks=(4096, 128, 256), vs=(4096, 128, 256), mbs=0, mrs=4096,
          B=1, H=2, T=2, S=4096, D=64, cus=256, inv=0.125, ds=1, dm=0)
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
REFUSALS = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=3), DTYPE, "not served"), (dict(ds=0), DTYPE, "not served"), (dict(dm=7), DTYPE, "unknown"),
    (dict(ds=1, dm=2), DTYPE, "pair"), (dict(T=0), SHAPE, "query rows"), (dict(T=17), SHAPE, "query rows"), (dict(D=96), SHAPE, "head size"),
    (dict(B=0), SHAPE, "positive"), (dict(S=-1), SHAPE, "positive"), (dict(qs=(4096, -128, 256)), SHAPE, "negative stride"),
    (dict(mrs=-1), SHAPE, "negative mask stride"), (dict(B=2 ** 40, H=2 ** 40), SHAPE, "overflows"), (dict(ks=(2 ** 61, 128, 256), B=4), SHAPE, "overflows"),
    (dict(q=None), NULL, "NULL"), (dict(out=None), NULL, "NULL"), (dict(out=K), ARG, "in-place"), (dict(out=M), ARG, "in-place"),
    (dict(ws=V), ARG, "in-place"), (dict(ws=OUT), ARG, "in-place"), (dict(wsb=8), UNSUPPORTED, "workspace too small"),
    (dict(ws=None), UNSUPPORTED, "workspace too small"), (dict(B=2 ** 20, H=2 ** 12, S=1, ks=(0, 0, 0), qs=(0, 0, 0), vs=(0, 0, 0)), UNSUPPORTED, "grid"),
    # the header's order, one fault of each later class behind the first; no mask: neither its dtype code nor its strides are looked at
    (dict(ds=3, T=0, q=None, out=K, wsb=0), DTYPE, ""), (dict(T=0, q=None, out=K, wsb=0), SHAPE, ""), (dict(q=None, out=K, wsb=0), NULL, ""),
    (dict(out=K, wsb=0), ARG, ""), (dict(m=None, dm=9, mrs=-1, wsb=0), UNSUPPORTED, ""),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(kw, code, text):
    a, L = dict(OK, **kw), _lib.lib()
    rc = L.fqd_attn_decode_fwd(a["q"], a["k"], a["v"], a["m"], a["out"], a["ws"], a["wsb"], *a["qs"], *a["ks"], *a["vs"], a["mbs"], a["mrs"],
                               a["B"], a["H"], a["T"], a["S"], a["D"], a["cus"], a["inv"], a["ds"], a["dm"], None)
    assert rc == code and text in L.fq_last_error().decode(), (rc, L.fq_last_error())


def test_the_workspace_entry_point_answers_and_refuses():
    L, nb, ns = _lib.lib(), ctypes.c_size_t(1), ctypes.c_int64(0)
    assert L.fqd_attn_decode_workspace(1, 2, 2, 64, 4096, 256, 1, ctypes.byref(nb), ctypes.byref(ns)) == 0
    assert ns.value > 1 and nb.value == 2 * ns.value * 2 * 66 * 4          # (m, l, acc[D]) in fp32 per real query row, head and chunk
    assert ops.attn_decode_workspace(64, 64, 1, 128, 4096, 256) == (0, 1)  # enough heads to fill the device: one chunk, no workspace
    for args, code in (((1, 2, 2, 64, 9, 0, 0), DTYPE), ((1, 2, 17, 64, 9, 0, 2), SHAPE), ((1, 2, 2, 80, 9, 0, 2), SHAPE)):
        assert L.fqd_attn_decode_workspace(*args, ctypes.byref(nb), ctypes.byref(ns)) == code
    assert L.fqd_attn_decode_workspace(1, 2, 2, 64, 9, 0, 2, None, None) == NULL
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_decode.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fqd_[a-z0-9_]+)\s*\(", src)) == set(_lib.DECODE_EXPORTS) and L.fq_version() == 7


@pytest.fixture
def cpu_route():
    llm_qat_amd.allow_cpu_tensors(True)
    yield
    llm_qat_amd.allow_cpu_tensors(False)


@pytest.mark.parametrize("dtype,kind", [(torch.bfloat16, "f32"), (torch.float16, "ds"), (torch.bfloat16, "none")])
def test_the_cpu_route_is_the_float64_chain_within_one_output_rounding(dtype, kind, cpu_route):
    """one rounding of the output is at most u |out| <= u sum p |v|: C_out <= 1, and 2^-10 for the route's fp32 softmax (2^-21 of u)"""
    T, S, D = 3, 77, 64                                                     # sqrt(64) = 8: the CPU's division is the device's product
    q, k, v = R.inputs(T, S, D, dtype, "cpu", signed_v=True, pool=S)
    mask = R.mask_of(kind, T, S, dtype, "cpu", pad=9)
    out = attention.decode_attention(q, k, v, mask, D)
    assert out.shape == (R.B, R.H, T, D) and out.transpose(1, 2).is_contiguous()
    assert R.c_out(out, *R.ref64(q, k, v, mask, R.inv_of(D))) <= 1 + 2.0 ** -10
    llm_qat_amd.allow_cpu_tensors(False)
    for bad, exc, text in ((dict(), RuntimeError, "allow_cpu_tensors"), (dict(q=q.clone().requires_grad_(True)), RuntimeError, "forward only"),
                           (dict(q=q.float()), TypeError, None), (dict(k=k[:, :1]), ValueError, None), (dict(q=q[..., :32]), ValueError, None),
                           (dict(mask=torch.zeros(R.B, 1, T, S + 1)), ValueError, None)):
        a = dict(dict(q=q, k=k, v=v, mask=mask), **bad)
        with pytest.raises(exc, match=text):
            attention.decode_attention(a["q"], a["k"], a["v"], a["mask"], D)


def test_fake_tensors_through_the_compiled_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, k = (torch.empty(2, n, 3 * 128, dtype=torch.float16, device="cuda").view(2, n, 3, 128).transpose(1, 2) for n in (4, 900))
        out = compiled.attn_decode_op(q, k, k, torch.empty(2, 1, 4, 900, device="cuda"), 0.1)
        assert out.shape == (2, 4, 3, 128) and out.dtype == torch.float16 and out.is_contiguous()
        with pytest.raises(ValueError):
            compiled.attn_decode_op(torch.empty(2, 3, 17, 128, dtype=torch.float16, device="cuda"), k, k, None, 0.1)


def test_install_and_convert_take_decode_and_leave_the_default_as_it_was(cpu_route):
    ns = _stub_namespace()
    parent = ns.LlamaAttention
    assert attention.install(ns) is parent and ns.LlamaAttention.fused_attn_decode is False
    ns.LlamaAttention = parent
    attention.install(ns, decode=True)
    assert ns.LlamaAttention.fused_attn_decode is True and issubclass(ns.LlamaAttention, parent)
    a, b = torch.nn.ModuleList([parent()]), torch.nn.ModuleList([parent()])
    assert attention.convert(a) == 1 and attention.convert(b, decode=True) == 1 and attention.convert(b) == 0
    assert type(a[0]) is not type(b[0]) and not a[0].fused_attn_decode and b[0].fused_attn_decode
    before, h, pos = dict(ops.decode_counts), torch.randn(1, 2, 32), torch.arange(2)[None]      # CPU tensors are not the device's: a counted fallback
    b[0].load_state_dict(a[0].state_dict())
    assert torch.equal(a[0](h, position_ids=pos)[0], b[0](h, position_ids=pos)[0])
    assert ops.decode_counts == dict(before, fallback=before["fallback"] + 1)
