"""CPU tier of the decode attention over a codes cache: the opt-in CPU route against the float64 reference, the
Python refusals, and the fqk_ entry points' refusals and their order through ctypes."""
import ctypes

import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, attention

import attn_decode_reference as R
import attn_kvdecode_reference as KR
from test_attn_softmax_cpu import _stub_namespace

BITS = {"int8": 8, "int4": 4}


def call(a, mask=None, D=64, **kw):
    a = dict(a, **kw)
    return attention.kv_decode_attention(a["q"], a["k_codes"], a["k_t2"], a["v_codes"], a["v_t2"], mask, D, num_bits=a.get("num_bits", 8),
                                         rotary=a["rotary"], key_positions=a["key_positions"])


@pytest.fixture
def cpu_route():
    llm_qat_amd.allow_cpu_tensors(True)
    yield
    llm_qat_amd.allow_cpu_tensors(False)


@pytest.mark.parametrize("container", ["int8", "int4"])
@pytest.mark.parametrize("T,S,D,dtype,kind,rot", [(3, 77, 64, torch.bfloat16, "f32", True), (1, 33, 128, torch.float16, "none", False)])
def test_the_cpu_route_is_the_float64_chain_within_one_output_rounding(container, T, S, D, dtype, kind, rot, cpu_route):
    """as decode_attention's CPU route: one rounding of the output (C_out <= 1) and 2^-10 for the fp32 softmax"""
    a = KR.inputs(T, S, D, dtype, container, "cpu", rot)
    mask = R.mask_of(kind, T, S, dtype, "cpu", pad=9)
    out = call(a, mask, D, num_bits=BITS[container])
    assert out.shape == (R.B, R.H, T, D) and out.transpose(1, 2).is_contiguous()
    assert KR.measure(out, a, mask, D, container, dtype) <= 1 + 2.0 ** -10


def test_the_refusals(cpu_route):
    a = KR.inputs(2, 9, 64, torch.bfloat16, "int8", "cpu")
    four = KR.inputs(2, 9, 64, torch.bfloat16, "int4", "cpu")
    wide = KR.inputs(17, 9, 64, torch.bfloat16, "int8", "cpu")
    for bad, exc, text in ((dict(q=a["q"].clone().requires_grad_(True)), RuntimeError, "forward only"), (dict(q=wide["q"]), ValueError, "T <= 16"),
                           (dict(q=a["q"].repeat(1, 1, 1, 2)[..., :96]), ValueError, "D in"), (dict(num_bits=4), TypeError, "int4 codes"),
                           (dict(k_codes=four["k_codes"], v_codes=four["v_codes"]), TypeError, "int8 codes"),
                           (dict(rotary=tuple(t[:8] for t in a["rotary"]), key_positions=None), ValueError, "S = 9 keys"),
                           (dict(rotary=None), ValueError, "key_positions without")):
        with pytest.raises(exc, match=text):
            call(a, **bad)
    ns = _stub_namespace()
    for fn, arg in ((attention.install, ns), (attention.convert, torch.nn.ModuleList([ns.LlamaAttention()]))):
        with pytest.raises(ValueError, match="decode=True"):
            fn(arg, kv_codes=True)


P0 = ctypes.addressof(ctypes.create_string_buffer(1 << 15))
Q, KC, KT, VC, VT, M, COS, SIN, POS, OUT, WS = (P0 + 2048 * i for i in range(11))
OK = dict(q=Q, kc=KC, kt=KT, vc=VC, vt=VT, m=M, cos=COS, sin=SIN, pos=POS, out=OUT, ws=WS, wsb=1 << 30, qs=(4096, 128, 256), ks=(4096, 64, 128),
          vs=(4096, 64, 128), kts=4096, vts=4096, mbs=0, mrs=4096, pbs=0, P=4096, B=1, H=2, T=2, S=4096, D=64, cus=256, inv=0.125, ds=1, dm=0, cb=8)
DTYPE, BITS_, SHAPE, NULL, ARG, UNSUPPORTED = -1, -2, -3, -4, -7, -8
REFUSALS = [
    (dict(ds=9), DTYPE, "unknown"), (dict(ds=0), DTYPE, "not served"), (dict(dm=7), DTYPE, "unknown"), (dict(dm=2), DTYPE, "pair"),
    (dict(cb=16), BITS_, "container"), (dict(T=17), SHAPE, "query rows"), (dict(D=96), SHAPE, "head size"), (dict(S=0), SHAPE, "positive"),
    (dict(ks=(4096, -64, 128)), SHAPE, "negative stride"), (dict(kts=-1), SHAPE, "negative stride of t2"), (dict(P=0), SHAPE, "table rows"),
    (dict(vs=(2 ** 61, 64, 128), B=4), SHAPE, "overflows"), (dict(kt=None), NULL, "NULL"), (dict(sin=None), NULL, "together"),
    (dict(cos=None, sin=None), NULL, "without the tables"), (dict(out=VC), ARG, "in-place"), (dict(ws=COS), ARG, "in-place"),
    (dict(ws=OUT), ARG, "in-place"), (dict(wsb=8), UNSUPPORTED, "workspace too small"),
    # the header's order, one fault of each later class behind the first
    (dict(ds=3, cb=5, T=0, q=None, out=KC, wsb=0), DTYPE, ""), (dict(cb=5, T=0, q=None, out=KC, wsb=0), BITS_, ""),
    (dict(T=0, q=None, out=KC, wsb=0), SHAPE, ""), (dict(q=None, out=KC, wsb=0), NULL, ""), (dict(out=KC, wsb=0), ARG, ""),
]


@pytest.mark.parametrize("kw,code,text", REFUSALS)
def test_every_refusal_comes_back_with_its_code_before_any_launch(kw, code, text):
    a, L = dict(OK, **kw), _lib.lib()
    rc = L.fqk_attn_kvdecode_fwd(a["q"], a["kc"], a["kt"], a["vc"], a["vt"], a["m"], a["cos"], a["sin"], a["pos"], a["out"], a["ws"], a["wsb"], *a["qs"],
                                 *a["ks"], *a["vs"], a["kts"], a["vts"], a["mbs"], a["mrs"], a["pbs"], a["P"], a["B"], a["H"], a["T"], a["S"], a["D"],
                                 a["cus"], a["inv"], a["ds"], a["dm"], a["cb"], None)
    assert rc == code and text in L.fq_last_error().decode(), (rc, L.fq_last_error())


def test_the_workspace_entry_point_is_the_decode_split():
    L, nb, ns = _lib.lib(), ctypes.c_size_t(1), ctypes.c_int64(0)
    assert all(hasattr(L, name) for name in _lib.KVDECODE_SYMBOLS) and L.fq_version() == 7
    assert L.fqk_attn_kvdecode_workspace(1, 2, 2, 64, 4096, 256, 1, 4, ctypes.byref(nb), ctypes.byref(ns)) == 0
    assert (nb.value, ns.value) == llm_qat_amd.ops.attn_decode_workspace(1, 2, 2, 64, 4096, 256) and ns.value > 1
    for args, code in (((1, 2, 2, 64, 9, 0, 0, 8), DTYPE), ((1, 2, 2, 64, 9, 0, 2, 3), BITS_), ((1, 2, 17, 64, 9, 0, 2, 8), SHAPE)):
        assert L.fqk_attn_kvdecode_workspace(*args, ctypes.byref(nb), ctypes.byref(ns)) == code
    assert L.fqk_attn_kvdecode_workspace(1, 2, 2, 64, 9, 0, 2, 8, None, None) == NULL
