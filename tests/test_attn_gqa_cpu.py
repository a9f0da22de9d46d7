"""CPU tier of grouped-query attention: the fqh_ entry points' refusals and their order through ctypes, the
header's names against _lib's list, the Python checks, and the opt-in CPU routes against the float64 reference."""
import ctypes
import os
import re

import pytest
import torch

import llm_qat_amd
from conftest import ROOT
from llm_qat_amd import _lib, attention, ops

import attn_decode_reference as R
import attn_kvdecode_reference as KR

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 15))
Q, KC, KT, VC, VT, M, COS, SIN, POS, OUT, WS = (P0 + 2048 * i for i in range(11))
OK = dict(q=Q, kc=KC, kt=KT, vc=VC, vt=VT, m=M, cos=COS, sin=SIN, pos=POS, out=OUT, ws=WS, wsb=1 << 30, qs=(8192, 128, 256), ks=(4096, 64, 128),
          vs=(4096, 64, 128), kts=4096, vts=4096, mbs=0, mrs=4096, pbs=0, P=4096, B=1, H=8, Hkv=2, T=2, S=4096, D=64, cus=256, inv=0.125, ds=1, dm=0,
          cb=8, causal=0)
DTYPE, BITS, SHAPE, NULL, ARG, UNSUPPORTED = -1, -2, -3, -4, -7, -8


def decode(a, L):
    return L.fqh_attn_decode_fwd(a["q"], a["kc"], a["vc"], a["m"], a["out"], a["ws"], a["wsb"], *a["qs"], *a["ks"], *a["vs"], a["mbs"], a["mrs"], a["B"],
                                 a["H"], a["Hkv"], a["T"], a["S"], a["D"], a["cus"], a["inv"], a["ds"], a["dm"], None)


def codes(a, L):
    return L.fqh_attn_kvdecode_fwd(a["q"], a["kc"], a["kt"], a["vc"], a["vt"], a["m"], a["cos"], a["sin"], a["pos"], a["out"], a["ws"], a["wsb"], *a["qs"],
                                   *a["ks"], *a["vs"], a["kts"], a["vts"], a["mbs"], a["mrs"], a["pbs"], a["P"], a["B"], a["H"], a["Hkv"], a["T"], a["S"],
                                   a["D"], a["cus"], a["inv"], a["ds"], a["dm"], a["cb"], None)


def prefill(a, L):
    return L.fqh_attn_prefill_fwd(a["q"], a["kc"], a["vc"], a["m"], a["out"], *a["qs"], *a["ks"], *a["vs"], a["mbs"], a["mrs"], a["B"], a["H"], a["Hkv"],
                                  a["T"], a["S"], a["D"], a["inv"], a["ds"], a["dm"], a["causal"], None)


EVERY = (decode, codes, prefill)
REFUSALS = [
    (EVERY, dict(ds=9), DTYPE, "unknown"), (EVERY, dict(ds=0), DTYPE, "not served"), (EVERY, dict(dm=2), DTYPE, "pair"), ((codes,), dict(cb=16), BITS, "container"),
    (EVERY, dict(S=0), SHAPE, "positive"), (EVERY, dict(Hkv=0), SHAPE, "K/V heads"), (EVERY, dict(Hkv=3), SHAPE, "divide"), (EVERY, dict(Hkv=-2), SHAPE, "K/V heads"),
    ((decode, codes), dict(T=17), SHAPE, "query rows"), (EVERY, dict(D=96), SHAPE, "head size"), (EVERY, dict(ks=(4096, -64, 128)), SHAPE, "negative stride"),
    # k's extent is over Hkv heads: a head stride that H = 8 heads would overflow with is served with Hkv = 2 (the next refusal is the NULL q)
    (EVERY, dict(ks=(4096, 2 ** 60, 128), q=None), NULL, "NULL"), (EVERY, dict(ks=(4096, 2 ** 60, 128), Hkv=8), SHAPE, "overflows"),
    (EVERY, dict(out=None), NULL, "NULL"), (EVERY, dict(out=VC), ARG, "in-place"), ((decode, codes), dict(ws=OUT), ARG, "in-place"),
    ((decode, codes), dict(wsb=8), UNSUPPORTED, "workspace too small"), ((decode, codes), dict(ws=None), UNSUPPORTED, "workspace too small"),
    ((prefill,), dict(causal=1), ARG, "causal together"), ((prefill,), dict(B=65536 // 8 + 1), UNSUPPORTED, "grid"),
    # the header's order, one fault of each later class behind the first
    (EVERY, dict(ds=3, Hkv=3, q=None, out=KC, wsb=0), DTYPE, ""), ((codes,), dict(cb=5, Hkv=3, q=None, out=KC, wsb=0), BITS, ""),
    (EVERY, dict(S=0, Hkv=3, T=17), SHAPE, "positive"), ((decode, codes), dict(Hkv=3, T=17), SHAPE, "divide"),
    (EVERY, dict(Hkv=3, q=None, out=KC, wsb=0), SHAPE, ""), (EVERY, dict(q=None, out=KC, wsb=0), NULL, ""), ((decode, codes), dict(out=KC, wsb=0), ARG, ""),
]


@pytest.mark.parametrize("fns,kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(fns, kw, code, text):
    L = _lib.lib()
    for fn in fns:
        rc = fn(dict(OK, **kw), L)
        assert rc == code and text in L.fq_last_error().decode(), (fn.__name__, rc, L.fq_last_error())


def test_the_header_the_list_and_the_workspace_split():
    L, nb, ns = _lib.lib(), ctypes.c_size_t(1), ctypes.c_int64(0)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_gqa.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fq[a-z0-9]*_[a-z0-9_]+)\s*\(", src)) == set(_lib.GQA_SYMBOLS) and all(hasattr(L, n) for n in _lib.GQA_SYMBOLS)
    assert L.fq_version() == 7
    # B Hkv NP workgroups ask the ungrouped split: G = 4 at T = 2 is one pack of 8 columns, at T = 8 two packs of two heads
    for T, wgs, cols in ((2, 2, 8), (8, 4, 16)):
        want_ns = ops.attn_decode_workspace(1, wgs, T, 64, 4096, 256)[1]
        want = (wgs * want_ns * cols * 66 * 4, want_ns)
        assert ops.attn_decode_workspace(1, 8, T, 64, 4096, 256, kv_heads=2) == want and want_ns > 1
        assert ops.attn_kvdecode_workspace(1, 8, T, 64, 4096, 256, num_bits=4, kv_heads=2) == want
    assert ops.attn_decode_workspace(1, 8, 2, 64, 4096, 256, kv_heads=8) == ops.attn_decode_workspace(1, 8, 2, 64, 4096, 256)
    for args, code in (((1, 8, 2, 2, 64, 9, 0, 0), DTYPE), ((1, 8, 3, 2, 64, 9, 0, 2), SHAPE), ((1, 8, 2, 17, 64, 9, 0, 2), SHAPE)):
        assert L.fqh_attn_decode_workspace(*args, ctypes.byref(nb), ctypes.byref(ns)) == code
    assert L.fqh_attn_kvdecode_workspace(1, 8, 2, 2, 64, 9, 0, 2, 3, ctypes.byref(nb), ctypes.byref(ns)) == BITS
    assert L.fqh_attn_decode_workspace(1, 8, 2, 2, 64, 9, 0, 2, None, None) == NULL


def gqa_inputs(T, S, D, dtype, G=4, Hkv=2):
    q, k, v = R.inputs(T, S, D, dtype, "cpu", H=Hkv * G, pool=128)
    return q, k[:, :Hkv], v[:, :Hkv]


def test_the_python_checks_accept_a_divisor_and_refuse_the_rest():
    q, k, v = gqa_inputs(2, 9, 64, torch.bfloat16)
    assert ops.check_attn_decode(q, k, v, None, 64)[:5] == (2, 8, 2, 9, 64) and ops.check_attn_prefill(q, k, v, None, 64, causal=True)[1] == 8
    codes = k.to(torch.int8)
    t2 = torch.ones(2, 9)
    assert ops.check_attn_kvdecode(q, codes, t2, codes, t2, None, 64)[:2] == (2, 8)
    for bad_k, bad_v in ((k[:, :0], v[:, :0]), (q[:, :3, :1].expand(2, 3, 9, 64), q[:, :3, :1].expand(2, 3, 9, 64)), (k, q[:, :4, :1].expand(2, 4, 9, 64))):
        with pytest.raises(ValueError, match="Hkv dividing H = 8"):
            ops.check_attn_decode(q, bad_k, bad_v, None, 64)
        with pytest.raises(ValueError, match="Hkv dividing H = 8"):
            ops.check_attn_kvdecode(q, bad_k.to(torch.int8), t2, bad_v.to(torch.int8), t2, None, 64)
    for fn in (ops.check_attn_train, attention.train_attention):
        with pytest.raises(ValueError, match="grouped-query"):
            fn(q, k, v, None, 64)


@pytest.mark.parametrize("T,S,D,dtype,kind", [(3, 77, 64, torch.bfloat16, "f32"), (1, 33, 128, torch.float16, "none")])
def test_the_cpu_routes_are_the_float64_chain_over_the_expanded_cache(T, S, D, dtype, kind):
    """as the ungrouped CPU routes: one rounding of the output (C_out <= 1) and 2^-10 for the fp32 softmax"""
    llm_qat_amd.allow_cpu_tensors(True)
    try:
        G = 4
        q, k, v = gqa_inputs(T, S, D, dtype, G)
        mask = R.mask_of(kind, T, S, dtype, "cpu", pad=9)
        ref, mag = R.ref64(q, k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), mask, R.inv_of(D))
        for out in (attention.decode_attention(q, k, v, mask, D), attention.prefill_attention(q, k, v, mask, D)):
            assert out.shape == q.shape and out.transpose(1, 2).is_contiguous() and R.c_out(out, ref, mag) <= 1 + 2.0 ** -10
        a = KR.inputs(T, S, D, dtype, "int8", "cpu", rot=True)      # KR.H = 3 query heads over the codes of head 0: G = 3
        wide = dict(a, k_codes=a["k_codes"][:, :1].repeat_interleave(3, 1), v_codes=a["v_codes"][:, :1].repeat_interleave(3, 1))
        out = attention.kv_decode_attention(a["q"], a["k_codes"][:, :1], a["k_t2"], a["v_codes"][:, :1], a["v_t2"], mask, D, rotary=a["rotary"],
                                            key_positions=a["key_positions"])
        assert KR.measure(out, wide, mask, D, "int8", dtype) <= 1 + 2.0 ** -10
    finally:
        llm_qat_amd.allow_cpu_tensors(False)
