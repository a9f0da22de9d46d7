"""CPU tier of the decode attention over an in-place K/V cache: the fqu_ entry points' refusals and their order
through ctypes, the header's names against _lib's list, the Python checks, the opt-in CPU route against the float64 reference at ragged
lengths, and static_kv_cache."""
import ctypes
import os
import re

import pytest
import torch

import llm_qat_amd
from conftest import ROOT
from llm_qat_amd import _lib, attention, ops

import attn_decode_reference as R

P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 20))
Q, KN, VN, LENS, OUT, WS = (P0 + 4096 * i for i in range(6))
KC, VC = P0 + (1 << 18), P0 + (1 << 19)      # 2 * 64 * 64 * 2 bytes each, apart from everything else
OK = dict(q=Q, kn=KN, vn=VN, kc=KC, vc=VC, lens=LENS, starts=None, out=OUT, ws=WS, wsb=1 << 30, qs=(1024, 128, 64), kns=(256, 128, 64), vns=(256, 128, 64),
          kcs=(8192, 4096, 64), vcs=(8192, 4096, 64), B=1, H=8, Hkv=2, T=2, Smax=64, D=64, cus=256, inv=0.125, ds=1)
DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8


def fwd(a, L):
    return L.fqu_attn_cached_fwd(a["q"], a["kn"], a["vn"], a["kc"], a["vc"], a["lens"], a["starts"], a["out"], a["ws"], a["wsb"], *a["qs"], *a["kns"], *a["vns"],
                                 *a["kcs"], *a["vcs"], a["B"], a["H"], a["Hkv"], a["T"], a["Smax"], a["D"], a["cus"], a["inv"], a["ds"], None)


BIG = dict(B=64, Smax=8192, kcs=(2 * 8192 * 64, 8192 * 64, 64), vcs=(2 * 8192 * 64, 8192 * 64, 64), kc=1 << 40, vc=1 << 41)      # nsplit > 1: a workspace is needed
REFUSALS = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=0), DTYPE, "not served"), (dict(Smax=0), SHAPE, "positive"), (dict(Hkv=3), SHAPE, "divide"),
    (dict(Hkv=0), SHAPE, "K/V heads"), (dict(T=17), SHAPE, "query rows"), (dict(D=96), SHAPE, "head size"), (dict(Smax=2 ** 31 - 2), SHAPE, "int32"),
    (dict(kcs=(8192, -4096, 64)), SHAPE, "negative stride"), (dict(kcs=(2 ** 62, 4096, 64), B=2), SHAPE, "overflows"),
    (dict(q=None), NULL, "NULL"), (dict(lens=None), NULL, "NULL"), (dict(kc=None), NULL, "NULL"), (dict(out=None), NULL, "NULL"),
    (dict(kn=KC + 8192), ARG, "overlaps a cache"), (dict(vn=VC - 2), ARG, "overlaps a cache"), (dict(q=VC + 16382), ARG, "overlaps a cache"),
    (dict(vc=KC), ARG, "one buffer"), (dict(out=KN), ARG, "in-place"), (dict(ws=LENS), ARG, "in-place"), (dict(ws=OUT), ARG, "in-place"),
    (dict(BIG, wsb=8), UNSUPPORTED, "workspace too small"), (dict(BIG, ws=None), UNSUPPORTED, "workspace too small"),
    # the header's order, one fault of each later class behind the first
    (dict(ds=3, Hkv=3, T=17, q=None, kn=KC, wsb=0), DTYPE, ""), (dict(Smax=0, Hkv=3, T=17), SHAPE, "positive"), (dict(Hkv=3, T=17, q=None), SHAPE, "divide"),
    (dict(T=17, q=None, kn=KC), SHAPE, "query rows"), (dict(q=None, kn=KC), NULL, ""), (dict(BIG, kn=(1 << 40) + 64, wsb=0), ARG, "overlaps"),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(kw, code, text):
    L = _lib.lib()
    rc = fwd(dict(OK, **kw), L)
    assert rc == code and text in L.fq_last_error().decode(), (rc, L.fq_last_error())


def test_the_header_the_list_and_the_static_workspace():
    L, nb, ns = _lib.lib(), ctypes.c_size_t(1), ctypes.c_int64(0)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn_cached.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fq[a-z0-9]*_[a-z0-9_]+)\s*\(", src)) == set(_lib.CACHED_SYMBOLS) and all(hasattr(L, n) for n in _lib.CACHED_SYMBOLS)
    assert L.fq_version() == 7
    # the grouped decode launch's split, asked with Smax: a function of the shapes alone
    for T in (2, 8):
        assert ops.attn_cached_workspace(1, 8, T, 64, 4096, 256, kv_heads=2) == ops.attn_decode_workspace(1, 8, T, 64, 4096, 256, kv_heads=2)
    assert ops.attn_cached_workspace(1, 8, 2, 64, 64, 256, kv_heads=2) == (0, 1)
    for args, code in (((1, 8, 2, 2, 64, 9, 0, 0), DTYPE), ((1, 8, 3, 2, 64, 9, 0, 2), SHAPE), ((1, 8, 2, 17, 64, 9, 0, 2), SHAPE)):
        assert L.fqu_attn_cached_workspace(*args, ctypes.byref(nb), ctypes.byref(ns)) == code
    assert L.fqu_attn_cached_workspace(1, 8, 2, 2, 64, 9, 0, 2, None, None) == NULL


def cached_inputs(lens, T, D, dtype, smax, G=2, Hkv=2):
    """-> q, k_new, v_new, caches with poison at and past each length, int32 lengths, and per batch row the (k, v) the reference attends over"""
    kc, vc = torch.full((len(lens), Hkv, smax, D), 2.0, dtype=dtype), torch.full((len(lens), Hkv, smax, D), 1024.0, dtype=dtype)
    qs, kn, vn, full = [], [], [], []
    for b, n in enumerate(lens):
        q, k, v = R.inputs(T, n + T, D, dtype, "cpu", seed=b, B=1, H=Hkv * G, pool=128)
        k, v = k[:, :Hkv], v[:, :Hkv]
        kc[b, :, :n], vc[b, :, :n] = k[0, :, :n], v[0, :, :n]
        qs.append(q), kn.append(k[:, :, n:]), vn.append(v[:, :, n:]), full.append((k, v))
    return torch.cat(qs), torch.cat(kn), torch.cat(vn), kc, vc, torch.tensor(lens, dtype=torch.int32), full


def test_the_python_checks():
    q, kn, vn, kc, vc, lens, _ = cached_inputs((3, 0), 2, 64, torch.bfloat16, 16)
    assert ops.check_attn_cached(q, kn, vn, kc, vc, lens, 64)[:6] == (2, 4, 2, 2, 16, 64)
    for bad, exc, text in ((dict(kn=kn.float()), TypeError, "all five"), (dict(lens=lens.long()), TypeError, "int32"), (dict(kn=kn[:, :, :1]), ValueError, "Hkv dividing H = 4"),
                           (dict(vn=vn[:, :1]), ValueError, "Hkv dividing"), (dict(vc=vc[:, :, :8]), ValueError, "Smax"), (dict(lens=lens[:1]), ValueError, r"cache_lens is \[2\]"),
                           (dict(kc=kc.transpose(2, 3).contiguous().transpose(2, 3)), ValueError, "not copied"), (dict(starts=lens[:, None]), ValueError, "cache_starts"),
                           (dict(q=q.new_zeros(2, 4, 17, 64)), ValueError, "T <= 16"), (dict(q=3), TypeError, "torch.Tensor")):
        a = dict(dict(q=q, kn=kn, vn=vn, kc=kc, vc=vc, lens=lens, starts=None), **bad)
        with pytest.raises(exc, match=text):
            ops.check_attn_cached(a["q"], a["kn"], a["vn"], a["kc"], a["vc"], a["lens"], 64, cache_starts=a["starts"])
    with pytest.raises(RuntimeError, match="no CPU"):
        attention.cached_decode_attention(q, kn, vn, kc, vc, lens, 64)
    with pytest.raises(RuntimeError, match="forward only"):
        attention.cached_decode_attention(q.clone().requires_grad_(True), kn, vn, kc, vc, lens, 64)


@pytest.mark.parametrize("lens,starts,T,D,dtype", [((0, 30, 61), None, 3, 64, torch.bfloat16), ((7, 47), (2, 33), 1, 128, torch.float16)])
def test_the_cpu_route_is_the_float64_chain_at_ragged_lengths(lens, starts, T, D, dtype):
    """as the other CPU routes: one rounding of the output (C_out <= 1) and 2^-10 for the fp32 softmax; the append bit for bit"""
    llm_qat_amd.allow_cpu_tensors(True)
    try:
        G, smax = 2, 64
        q, kn, vn, kc, vc, dl, full = cached_inputs(lens, T, D, dtype, smax, G)
        want = (kc.clone(), vc.clone())
        for b, n in enumerate(lens):
            want[0][b, :, n:n + T], want[1][b, :, n:n + T] = kn[b], vn[b]
        out = attention.cached_decode_attention(q, kn, vn, kc, vc, dl, D, cache_starts=None if starts is None else torch.tensor(starts, dtype=torch.int32))
        assert out.shape == q.shape and out.transpose(1, 2).is_contiguous() and torch.equal(kc, want[0]) and torch.equal(vc, want[1])
        for b, (k, v) in enumerate(full):
            mask = R.mask_of("ds", T, k.shape[2], dtype, "cpu", batch=1, pad=0 if starts is None else starts[b])
            ref, mag = R.ref64(q[b:b + 1], k.repeat_interleave(G, 1), v.repeat_interleave(G, 1), mask, R.inv_of(D))
            assert R.c_out(out[b:b + 1], ref, mag) <= 1 + 2.0 ** -10, b
    finally:
        llm_qat_amd.allow_cpu_tensors(False)


def test_static_kv_cache_holds_the_prompt_and_its_length():
    k, v = torch.randn(2, 3, 5, 64).bfloat16(), torch.randn(2, 3, 5, 64).bfloat16()
    kc, vc, lens = attention.static_kv_cache(k.transpose(1, 2).contiguous().transpose(1, 2), v, 12)
    assert kc.shape == vc.shape == (2, 3, 12, 64) and kc.is_contiguous() and kc.dtype == k.dtype
    assert torch.equal(kc[:, :, :5], k) and torch.equal(vc[:, :, :5], v) and not kc[:, :, 5:].any() and not vc[:, :, 5:].any()
    assert lens.dtype == torch.int32 and lens.tolist() == [5, 5]
    with pytest.raises(ValueError, match="below the prompt"):
        attention.static_kv_cache(k, v, 4)
    assert "cached_decode_attention" not in attention.__all__ and "static_kv_cache" not in attention.__all__
