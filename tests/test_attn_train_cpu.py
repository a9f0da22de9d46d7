"""CPU tier of the fused training attention: every refusal of fqg_attn_train_fwd and fqg_attn_train_bwd through
ctypes and their order, the opt-in CPU route's result and gradients against the float64 reference, the Python refusals, fake tensors
through both compiled ops, install / convert with and without train."""
import ctypes
import os
import re

import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, attention, compiled, ops

import attn_train_reference as R
from conftest import ROOT
from test_attn_softmax_cpu import _stub_namespace

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 15))
Q, K, V, M, OUT, DOUT, STATS, DELTA, DQ, DK, DV = (P0 + 2048 * i for i in range(11))
ST = (4096, 128, 256)
OK = dict(q=Q, k=K, v=V, m=M, out=OUT, dout=DOUT, stats=STATS, delta=DELTA, dq=DQ, dk=DK, dv=DV, qs=ST, ks=ST, vs=ST, os=ST, gs=ST, mbs=0,
          mrs=4096, B=1, H=2, T=200, S=4096, D=64, inv=0.125, ds=1, dm=0, causal=0)
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
BOTH = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=3), DTYPE, "not served"), (dict(ds=0), DTYPE, "not served"), (dict(dm=7), DTYPE, "unknown"),
    (dict(ds=1, dm=2), DTYPE, "pair"), (dict(T=0), SHAPE, "positive"), (dict(D=96), SHAPE, "head size"), (dict(S=-1), SHAPE, "positive"),
    (dict(qs=(4096, -128, 256)), SHAPE, "negative stride"), (dict(mrs=-1), SHAPE, "negative mask stride"),
    (dict(B=2 ** 40, H=2 ** 40), SHAPE, "overflows"), (dict(ks=(2 ** 61, 128, 256), B=4), SHAPE, "overflows"),
    (dict(m=None, causal=1, T=4097), SHAPE, "causal"), (dict(q=None), NULL, "NULL"), (dict(out=None), NULL, "NULL"),
    (dict(causal=1), ARG, "causal together with a mask"),
    (dict(B=2 ** 10, H=2 ** 7, T=1, S=1, ks=(0, 0, 0), qs=(0, 0, 0), vs=(0, 0, 0), os=(0, 0, 0), gs=(0, 0, 0)), UNSUPPORTED, "grid"),
    # the header's order, one fault of each later class behind the first
    (dict(ds=3, T=0, q=None, causal=1, B=2 ** 17), DTYPE, ""), (dict(T=0, q=None, causal=1, B=2 ** 17), SHAPE, ""),
    (dict(q=None, causal=1, B=2 ** 17), NULL, ""), (dict(causal=1, B=2 ** 17), ARG, ""), (dict(m=None, dm=9, mrs=-1, B=2 ** 17), UNSUPPORTED, ""),
]
FWD = [(dict(out=K), ARG, "in-place"), (dict(stats=M), ARG, "in-place"), (dict(stats=OUT), ARG, "one pointer")]
BWD = [(dict(gs=(4096, 128, -1)), SHAPE, "negative stride"), (dict(os=(2 ** 61, 128, 256), B=4), SHAPE, "overflows"), (dict(dout=None), NULL, "NULL"),
       (dict(stats=None), NULL, "NULL"), (dict(delta=None), NULL, "NULL"), (dict(dk=None), NULL, "NULL"), (dict(dq=K), ARG, "in-place"),
       (dict(delta=STATS), ARG, "in-place"), (dict(dv=DOUT), ARG, "in-place"), (dict(dk=DV), ARG, "one pointer")]


def call(entry, a):
    L = _lib.lib()
    if entry == "fwd":
        return L.fqg_attn_train_fwd(a["q"], a["k"], a["v"], a["m"], a["out"], a["stats"], *a["qs"], *a["ks"], *a["vs"], a["mbs"], a["mrs"],
                                    a["B"], a["H"], a["T"], a["S"], a["D"], a["inv"], a["ds"], a["dm"], a["causal"], None)
    return L.fqg_attn_train_bwd(a["q"], a["k"], a["v"], a["m"], a["out"], a["dout"], a["stats"], a["delta"], a["dq"], a["dk"], a["dv"], *a["qs"],
                                *a["ks"], *a["vs"], *a["os"], *a["gs"], a["mbs"], a["mrs"], a["B"], a["H"], a["T"], a["S"], a["D"], a["inv"],
                                a["ds"], a["dm"], a["causal"], None)


@pytest.mark.parametrize("entry,kw,code,text", [("fwd", *r) for r in BOTH + FWD] + [("bwd", *r) for r in BOTH + BWD])
def test_every_refusal_comes_back_with_its_code_before_any_launch(entry, kw, code, text):
    rc = call(entry, dict(OK, **kw))
    assert rc == code and text in _lib.lib().fq_last_error().decode(), (rc, _lib.lib().fq_last_error())


def test_the_header_declares_the_exports_and_no_other_set_has_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_train.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fqg_[a-z0-9_]+)\s*\(", src)) == set(_lib.ATTN_TRAIN_EXPORTS) and _lib.lib().fq_version() == 7
    others = [v for n, v in vars(_lib).items() if n.endswith("EXPORTS") and n != "ATTN_TRAIN_EXPORTS"]
    assert len(others) == 12 and not set(_lib.ATTN_TRAIN_EXPORTS) & {s for v in others for s in v}


@pytest.fixture
def cpu_route():
    llm_qat_amd.allow_cpu_tensors(True)
    yield
    llm_qat_amd.allow_cpu_tensors(False)


@pytest.mark.parametrize("dtype,kind", [(torch.bfloat16, "f32"), (torch.float16, "ds"), (torch.bfloat16, "none"), (torch.float16, "causal")])
def test_the_cpu_route_is_the_float64_reference_within_one_rounding(dtype, kind, cpu_route):
    """one rounding of a result x is at most u |x|, and |x| is at most its measure's magnitude: every C <= 1 (2^-10: the arithmetic of two
    float64 formulations)"""
    T, S, D = 37, 77, 64                                                    # sqrt(64) = 8: the CPU's division is the device's product
    q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, "cpu")
    dout = R.dout_of(T, D, dtype, "cpu")
    got = R.fused(q, k, v, mask, D, dout, causal)
    assert got["out"].shape == (R.B, R.H, T, D) and got["out"].transpose(1, 2).is_contiguous() and got["dk"].dtype == dtype
    c = R.measures(got, R.ref64(q, k, v, ref_mask, R.inv_of(D), dout))
    assert max(c.values()) <= 1 + 2.0 ** -10, c
    llm_qat_amd.allow_cpu_tensors(False)
    for bad, exc, text in ((dict(), RuntimeError, "allow_cpu_tensors"), (dict(mask=torch.zeros(R.B, 1, T, S, requires_grad=True)), ValueError, "requires grad"),
                           (dict(mask=torch.zeros(R.B, 1, T, S), causal=True), ValueError, "causal"), (dict(k=k[:, :, :5], v=v[:, :, :5], causal=True), ValueError, "T <= S"),
                           (dict(causal=1), TypeError, "bool"), (dict(q=q.float()), TypeError, None), (dict(q=q[..., :32]), ValueError, None)):
        a = dict(dict(q=q, k=k, v=v, mask=None, causal=False), **bad)
        with pytest.raises(exc, match=text):
            attention.train_attention(a["q"], a["k"], a["v"], a["mask"], D, causal=a["causal"])


def test_fake_tensors_through_both_compiled_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, k = (torch.empty(2, n, 3 * 128, dtype=torch.float16, device="cuda").view(2, n, 3, 128).transpose(1, 2) for n in (400, 900))
        mask = torch.empty(2, 1, 400, 900, device="cuda")
        out, stats = compiled.attn_train_fwd_op(q, k, k, mask, 0.1, False, True)
        assert out.shape == (2, 400, 3, 128) and out.dtype == torch.float16 and out.is_contiguous() and stats.shape == (2, 3, 400, 2)
        assert compiled.attn_train_fwd_op(q, k, k, None, 0.1, True, False)[1].shape == (0, 2)
        dq, dk, dv = compiled.attn_train_bwd_op(torch.empty_like(out), q, k, k, mask, out, stats, 0.1, False)
        assert dq.shape == out.shape and dk.shape == dv.shape == (2, 900, 3, 128) and dk.is_contiguous() and dk.dtype == torch.float16
        with pytest.raises(ValueError):
            compiled.attn_train_fwd_op(k, q, q, None, 0.1, True, True)


def test_install_and_convert_take_train_and_leave_the_defaults_as_they_were(cpu_route):
    ns = _stub_namespace()
    parent = ns.LlamaAttention
    assert attention.install(ns) is parent and ns.LlamaAttention.fused_attn_train is False and ns.LlamaAttention.fused_attn_prefill is False
    ns.LlamaAttention = parent
    attention.install(ns, train=True)
    assert ns.LlamaAttention.fused_attn_train is True and ns.LlamaAttention.fused_attn_decode is False and issubclass(ns.LlamaAttention, parent)
    a, b, c, d = (torch.nn.ModuleList([parent()]) for _ in range(4))
    assert attention.convert(a) == 1 and attention.convert(b, train=True) == 1 and attention.convert(c, prefill=True, train=True) == 1
    assert attention.convert(d, train=True) == 1 and type(d[0]) is type(b[0]) and len({type(a[0]), type(b[0]), type(c[0])}) == 3
    assert not a[0].fused_attn_train and b[0].fused_attn_train and not b[0].fused_attn_prefill and c[0].fused_attn_prefill
    h, pos = torch.randn(1, 2, 32), torch.arange(2)[None]                   # CPU tensors are not the device's: counted fallbacks, the three calls
    for m, pre, trn in ((a[0], 0, 0), (b[0], 0, 1), (c[0], 1, 1)):
        before = dict(ops.decode_counts), dict(ops.prefill_counts), dict(ops.train_counts)
        m.load_state_dict(a[0].state_dict())
        assert torch.equal(a[0](h, position_ids=pos)[0], m(h, position_ids=pos)[0])       # the parameters require grad
        assert ops.decode_counts == before[0] and ops.prefill_counts == dict(before[1], fallback=before[1]["fallback"] + pre)
        assert ops.train_counts == dict(before[2], fallback=before[2]["fallback"] + trn)
        with torch.no_grad():
            m(h, position_ids=pos)
        assert ops.train_counts["fallback"] == before[2]["fallback"] + trn      # a call that needs no gradient is not the train route's
    assert attention.__all__ == ["attn_softmax", "install", "convert"]
