"""CPU tier of the decode attention over an in-place K/V cache of integer codes: the fqw_ entry points' refusals
and their order through ctypes, the header's names against _lib's list, the Python checks, the opt-in CPU route against the float64
reference at ragged lengths, and static_kv_codes_cache."""
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

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 20))
Q, KN, KTN, VN, VTN, LENS, OUT, WS, COS, SIN = (P0 + 4096 * i for i in range(10))
KC, VC, KTC, VTC = (P0 + (1 << 17) * i for i in range(2, 6))      # 2 * 64 * 64 bytes of codes or 64 * 4 of divisors each, apart from everything else
OK = dict(q=Q, kn=KN, ktn=KTN, vn=VN, vtn=VTN, kc=KC, ktc=KTC, vc=VC, vtc=VTC, lens=LENS, starts=None, cos=None, sin=None, out=OUT, ws=WS, wsb=1 << 30,
          qs=(1024, 128, 64), kns=(256, 128, 64), vns=(256, 128, 64), kcs=(8192, 4096, 64), vcs=(8192, 4096, 64), t2s=(2, 2, 64, 64), P=0, B=1, H=8, Hkv=2, T=2,
          Smax=64, D=64, cus=256, inv=0.125, ds=1, bits=8)
DTYPE, BITS, SHAPE, NULL, ARG, UNSUPPORTED = -1, -2, -3, -4, -7, -8


def fwd(a, L):
    return L.fqw_attn_cached_codes_fwd(a["q"], a["kn"], a["ktn"], a["vn"], a["vtn"], a["kc"], a["ktc"], a["vc"], a["vtc"], a["lens"], a["starts"], a["cos"], a["sin"],
                                       a["out"], a["ws"], a["wsb"], *a["qs"], *a["kns"], *a["vns"], *a["kcs"], *a["vcs"], *a["t2s"], a["P"], a["B"], a["H"], a["Hkv"],
                                       a["T"], a["Smax"], a["D"], a["cus"], a["inv"], a["ds"], a["bits"], None)


BIG = dict(B=64, Smax=8192, kcs=(2 * 8192 * 64, 8192 * 64, 64), vcs=(2 * 8192 * 64, 8192 * 64, 64), t2s=(2, 2, 8192, 8192), kc=1 << 40, vc=1 << 41, ktc=1 << 42,
           vtc=1 << 43)      # nsplit > 1: a workspace is needed
REFUSALS = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=0), DTYPE, "not served"), (dict(bits=6), BITS, "container"), (dict(Smax=0), SHAPE, "positive"),
    (dict(Hkv=3), SHAPE, "divide"), (dict(T=17), SHAPE, "query rows"), (dict(D=96), SHAPE, "head size"), (dict(Smax=2 ** 31 - 2), SHAPE, "int32"),
    (dict(kcs=(8192, -4096, 64)), SHAPE, "negative stride"), (dict(t2s=(2, 2, -1, 64)), SHAPE, "negative stride"), (dict(cos=COS, sin=SIN), SHAPE, "table rows"),
    (dict(kcs=(2 ** 61, 4096, 64), B=2), SHAPE, "overflows"), (dict(q=None), NULL, "NULL"), (dict(ktn=None), NULL, "NULL"), (dict(vtc=None), NULL, "NULL"),
    (dict(lens=None), NULL, "NULL"), (dict(cos=COS, P=64), NULL, "together"), (dict(kn=KC + 8000), ARG, "overlaps a cache"), (dict(vtn=VTC + 252), ARG, "overlaps a cache"),
    (dict(q=VC - 2), ARG, "overlaps a cache"), (dict(vc=KC + 8191), ARG, "two caches"), (dict(vtc=KTC), ARG, "two caches"), (dict(out=KTN), ARG, "in-place"),
    (dict(ws=LENS), ARG, "in-place"), (dict(ws=OUT), ARG, "in-place"), (dict(BIG, wsb=8), UNSUPPORTED, "workspace too small"),
    (dict(BIG, ws=None), UNSUPPORTED, "workspace too small"),
    # the header's order, one fault of each later class behind the first
    (dict(ds=3, bits=5, Hkv=3, q=None, kn=KC, wsb=0), DTYPE, ""), (dict(bits=5, Smax=0, q=None), BITS, ""), (dict(Hkv=3, T=17, q=None), SHAPE, "divide"),
    (dict(T=17, q=None, kn=KC), SHAPE, "query rows"), (dict(q=None, kn=KC), NULL, ""), (dict(BIG, kn=(1 << 40) + 64, wsb=0), ARG, "overlaps"),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(kw, code, text):
    L = _lib.lib()
    rc = fwd(dict(OK, **kw), L)
    assert rc == code and text in L.fq_last_error().decode(), (rc, L.fq_last_error())


def test_the_header_the_list_and_the_static_workspace():
    L, nb, ns = _lib.lib(), ctypes.c_size_t(1), ctypes.c_int64(0)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_cached_codes.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(fq[a-z0-9]*_[a-z0-9_]+)\s*\(", src))
    assert names == set(_lib.CACHED_CODES_SYMBOLS) and all(hasattr(L, n) for n in names) and L.fq_version() == 7
    for bits in (8, 4):      # the in-place cache's split, whatever the container: a function of the shapes alone
        assert ops.attn_cached_codes_workspace(1, 8, 2, 64, 4096, 256, num_bits=bits, kv_heads=2) == ops.attn_cached_workspace(1, 8, 2, 64, 4096, 256, kv_heads=2)
    assert ops.attn_cached_codes_workspace(1, 8, 2, 64, 64, 256, kv_heads=2) == (0, 1)
    for args, code in (((1, 8, 2, 2, 64, 9, 0, 0, 8), DTYPE), ((1, 8, 2, 2, 64, 9, 0, 2, 3), BITS), ((1, 8, 3, 2, 64, 9, 0, 2, 8), SHAPE)):
        assert L.fqw_attn_cached_codes_workspace(*args, ctypes.byref(nb), ctypes.byref(ns)) == code
    assert L.fqw_attn_cached_codes_workspace(1, 8, 2, 2, 64, 9, 0, 2, 8, None, None) == NULL


NAMES = ("k_codes", "k_t2", "v_codes", "v_t2")


def cached_inputs(lens, T, D, dtype, container, smax, G):
    """KR.inputs (B = 2, H = 3 K/V heads) cut at each length -> q of 3 G heads, the new tensors, caches with poison (the largest code over
    2^-3) at and past each length, the int32 lengths, the source tensors and the tables"""
    a = KR.inputs(T, smax + T, D, dtype, container, "cpu", seed=5)
    q = (torch.randint(-8, 9, (KR.B, KR.H * G, T, D), generator=torch.Generator().manual_seed(G)).float() / 4).to(dtype)
    new, caches = {}, {}
    for n in NAMES:
        t = a[n].contiguous()
        key = 2 if t.dim() == 4 else 1      # the key axis
        new[n] = torch.stack([t[b].narrow(key - 1, hi, T) for b, hi in enumerate(lens)])
        caches[n] = torch.full_like(t.narrow(key, 0, smax), 0.125 if t.dim() == 2 else 0x77 if container == "int4" else 127)
        for b, hi in enumerate(lens):
            caches[n][b].narrow(key - 1, 0, hi).copy_(t[b].narrow(key - 1, 0, hi))
    return q, new, caches, torch.tensor(lens, dtype=torch.int32), a


def call(q, new, caches, lens, D, **kw):
    return attention.cached_kv_decode_attention(q, *(new[n] for n in NAMES), *(caches[n] for n in NAMES), lens, D, **kw)


def test_the_python_checks_and_the_refusals_of_cpu_tensors_and_gradients():
    q, new, caches, lens, a = cached_inputs((3, 0), 2, 64, torch.bfloat16, "int8", 16, 2)
    args = dict(q=q, **{n + "_new": new[n] for n in NAMES}, **{n + "_cache": caches[n] for n in NAMES}, lens=lens, starts=None, bits=8, rotary=None)

    def check(**bad):
        x = dict(args, **bad)
        return ops.check_attn_cached_codes(x["q"], *(x[n + "_new"] for n in NAMES), *(x[n + "_cache"] for n in NAMES), x["lens"], 64, num_bits=x["bits"],
                                           rotary=x["rotary"], cache_starts=x["starts"])
    assert check()[:6] == (2, 6, 3, 2, 16, 64) and check()[7:] == ("int8", 0) and check(rotary=a["rotary"])[8] == 18
    kc, tables = caches["k_codes"], a["rotary"]
    for bad, exc, text in ((dict(q=3), TypeError, "torch.Tensor"), (dict(q=q.float()), TypeError, "bfloat16 or float16"), (dict(bits=4), TypeError, "int4 codes"),
                           (dict(k_t2_new=new["k_t2"].double()), TypeError, "float32"), (dict(lens=lens.long()), TypeError, "int32"), (dict(rotary=tables[0]), TypeError, "pair"),
                           (dict(bits=9), ValueError, "1 .. 8"), (dict(q=q.new_zeros(2, 6, 17, 64)), ValueError, "T <= 16"), (dict(v_codes_new=new["v_codes"][:, :1]), ValueError, "Hkv dividing"),
                           (dict(v_t2_new=new["v_t2"][:, :1]), ValueError, "new divisors"), (dict(v_codes_cache=caches["v_codes"][:, :, :8]), ValueError, "Smax"),
                           (dict(k_t2_cache=caches["k_t2"][:, :8]), ValueError, "divisor caches"), (dict(k_codes_cache=kc.transpose(2, 3).contiguous().transpose(2, 3)), ValueError, "not copied"),
                           (dict(starts=lens[:, None]), ValueError, "cache_starts"), (dict(rotary=tuple(t[:15] for t in tables)), ValueError, "Smax = 16 rows")):
        with pytest.raises(exc, match=text):
            check(**bad)
    with pytest.raises(RuntimeError, match="no CPU"):
        call(q, new, caches, lens, 64)
    with pytest.raises(RuntimeError, match="forward only"):
        call(q.clone().requires_grad_(True), new, caches, lens, 64)


@pytest.mark.parametrize("lens,starts,T,D,dtype,container", [((0, 30), None, 3, 64, torch.bfloat16, "int4"), ((47, 7), (33, 2), 1, 128, torch.float16, "int8")])
def test_the_cpu_route_is_the_float64_chain_at_ragged_lengths(lens, starts, T, D, dtype, container):
    """as the other CPU routes: one rounding of the output (C_out <= 1) and 2^-10 for the fp32 softmax; the append bit for bit"""
    llm_qat_amd.allow_cpu_tensors(True)
    try:
        G, smax = 2, 48
        q, new, caches, dl, a = cached_inputs(lens, T, D, dtype, container, smax, G)
        want = {n: caches[n].clone() for n in NAMES}
        for n in NAMES:
            for b, hi in enumerate(lens):
                want[n][b].narrow(want[n].dim() - 3, hi, T).copy_(new[n][b])
        out = call(q, new, caches, dl, D, num_bits=4 if container == "int4" else 8, rotary=a["rotary"], cache_starts=None if starts is None else torch.tensor(starts, dtype=torch.int32))
        assert out.shape == q.shape and out.transpose(1, 2).is_contiguous() and all(torch.equal(caches[n], want[n]) for n in NAMES)
        for b, hi in enumerate(lens):
            S, lo = hi + T, 0 if starts is None else starts[b]
            pos = (torch.arange(S) - lo).clamp(min=0)[None]
            k, v = KR.operands(*(a[n][b:b + 1].narrow(2 if a[n].dim() == 4 else 1, 0, S) for n in NAMES), container, dtype, a["rotary"], pos)
            ref, mag = R.ref64(q[b:b + 1], k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), R.mask_of("ds", T, S, dtype, "cpu", batch=1, pad=lo), R.inv_of(D))
            assert R.c_out(out[b:b + 1], ref, mag.clamp(min=2.0 ** -20)) <= 1 + 2.0 ** -10, b
    finally:
        llm_qat_amd.allow_cpu_tensors(False)


def test_static_kv_codes_cache_holds_the_prompt_and_its_length():
    a = KR.inputs(1, 5, 64, torch.bfloat16, "int4", "cpu")
    kc, kt, vc, vt, lens = attention.static_kv_codes_cache(*(a[n] for n in NAMES), 12)
    assert kc.shape == vc.shape == (KR.B, KR.H, 12, 32) and kc.is_contiguous() and kc.dtype == torch.uint8 and kt.shape == vt.shape == (KR.B, 12)
    assert torch.equal(kc[:, :, :5], a["k_codes"]) and torch.equal(vc[:, :, :5], a["v_codes"]) and not kc[:, :, 5:].any() and not vc[:, :, 5:].any()
    assert torch.equal(kt[:, :5], a["k_t2"]) and torch.equal(vt[:, :5], a["v_t2"]) and (kt[:, 5:] == 1).all() and (vt[:, 5:] == 1).all()
    assert lens.dtype == torch.int32 and lens.tolist() == [5, 5]
    with pytest.raises(ValueError, match="below the prompt"):
        attention.static_kv_codes_cache(*(a[n] for n in NAMES), 4)
    assert "cached_kv_decode_attention" not in attention.__all__ and "static_kv_codes_cache" not in attention.__all__
