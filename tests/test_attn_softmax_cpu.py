"""CPU tier of the fused attention softmax (llm_qat_amd.attention): the opt-in CPU route against the reference's own
bits (tests/golden/attn_softmax.npz), the float64 reference against the fixture and against autograd, every refusal of the C ABI walked
through ctypes without a GPU, the compiled ops on fake tensors, install / convert on a stub namespace.  No kernel is launched here."""
import ctypes
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import llm_qat_amd
from llm_qat_amd import _lib, attention, compiled, ops, rope

import attn_softmax_reference as R
from conftest import GOLDEN, ROOT

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
FIX = np.load(os.path.join(GOLDEN, "attn_softmax.npz"))
HEAD_DIM = int(FIX["head_dim"])
NAMES = sorted({k.rsplit("_", 1)[0] for k in FIX.files if k.endswith("_scores")})


def load(name, field):
    ds, dm = name.split("_")[:2]
    a = FIX[f"{name}_{field}"]
    dt = DT[dm] if field == "mask" else DT[ds]
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy())
    return t.view(dt) if a.dtype == np.uint16 else t


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture
def cpu_route():
    llm_qat_amd.allow_cpu_tensors(True)
    yield
    llm_qat_amd.allow_cpu_tensors(False)


def test_the_fixture_holds_every_case_the_issue_lists():
    assert len(NAMES) == 15 and {n.split("_")[2] for n in NAMES} == {"causal", "padded", "past"}
    assert {tuple(n.split("_")[:2]) for n in NAMES} == {("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"), ("f32", "f32")}
    m = load("bf16_bf16_padded", "mask")
    assert (m[1, 0, 1] == float("-inf")).all() and (m[1, 0, 0] <= torch.finfo(torch.bfloat16).min).all()      # a -inf row, a fully masked row
    assert load("f32_f32_past", "scores").shape[-1] != load("f32_f32_past", "scores").shape[-2]


@pytest.mark.parametrize("name", NAMES)
def test_the_cpu_route_equals_the_references_bits(name, cpu_route):
    x, mask, gy = load(name, "scores").requires_grad_(True), load(name, "mask"), load(name, "gy")
    y = attention.attn_softmax(x, mask, HEAD_DIM)
    y.backward(gy)
    assert y.dtype == x.dtype and torch.equal(bits(y), bits(load(name, "y")))
    assert torch.equal(bits(x.grad), bits(load(name, "dscores")))


@pytest.mark.parametrize("name", NAMES)
def test_ref64_is_within_the_caps_of_the_fixture(name):
    x, mask, gy = load(name, "scores"), load(name, "mask"), load(name, "gy")
    ref = R.ref64(x, mask, gy, HEAD_DIM)
    cy, cdx = R.c_y(load(name, "y"), ref), R.c_dx(load(name, "dscores"), ref)
    print(name, "C_y", cy, "C_dx", cdx)
    assert cy <= R.Y_CAP and cdx <= R.DX_CAP


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("f32")] + ["bf16_f32_padded", "f16_f16_padded"])
def test_the_float64_recipe_equals_float64_autograd_of_the_chain(name):
    """tie rows (d / 2) and -inf rows (0) included: the chain itself in float64, differentiated by autograd"""
    x, mask, gy = load(name, "scores"), load(name, "mask"), load(name, "gy")
    ref = R.ref64(x, mask, gy, HEAD_DIM)
    scale = ref["inv"] * ref["p"] * (ref["g"].abs() + (ref["g"] * ref["p"]).abs().sum(-1, keepdim=True))      # what the terms that cancel are made of
    assert ((R.recipe64(ref) - ref["dx"]).abs() <= 1e-13 * scale).all()
    a = ref["a"].clone().requires_grad_(True)
    z = torch.max(a, torch.tensor(ref["min"], dtype=torch.float64))
    (da,) = torch.autograd.grad(torch.softmax(z, -1), a, ref["g"])
    assert torch.equal(da * ref["inv"], ref["dx"])
    if "padded" in name:
        assert (ref["dx"][1, :, 1] == 0).all()                      # the -inf row: below the clamp, no gradient
        if "_f32_" in name:                                         # (an fp16 sum min + x can round above min: no tie there)
            assert (ref["a"][1, :, 0] <= ref["min"]).all()          # a fully masked row: ties (and -inf elements)


def test_the_header_names_equal_the_exports_and_the_library_has_them():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llmqat_fakequant_attn.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fqs2_[a-z0-9_]+)\s*\(", src)) == set(_lib.ATTN_EXPORTS)
    L = _lib.lib()
    for n in _lib.ATTN_EXPORTS:
        assert hasattr(L, n)
    assert L.fq_version() == 7


# ---- refusals of the C ABI, before any HIP call -------------------------------------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(1 << 14)
P0 = ctypes.addressof(_BUF)
X, M, Y, ST, G = P0, P0 + 2048, P0 + 4096, P0 + 6144, P0 + 8192
OK_SHAPE = dict(rows=8, cols=16, B=1, H=2, T=4, mbs=0, mrs=16, inv=0.125, ds=1, dm=0)


def call(which, **kw):
    a = dict(OK_SHAPE, x=X, m=M, y=Y, st=ST, g=G)
    a.update(kw)
    L = _lib.lib()
    tail = (a["rows"], a["cols"], a["B"], a["H"], a["T"], a["mbs"], a["mrs"], a["inv"], a["ds"], a["dm"], None)
    if which == "fwd":
        return L.fqs2_attn_softmax_fwd(a["x"], a["m"], a["y"], a["st"], *tail), L.fq_last_error().decode()
    return L.fqs2_attn_softmax_bwd(a["g"], a["x"], a["m"], a["st"], a["y"], *tail), L.fq_last_error().decode()


DTYPE, SHAPE, NULL, ARG, UNSUPPORTED = -1, -3, -4, -7, -8
BOTH = [
    (dict(ds=3), DTYPE, "float64"), (dict(ds=9), DTYPE, "unknown"), (dict(dm=3), DTYPE, "float64"), (dict(ds=1, dm=2), DTYPE, "pair"),
    (dict(ds=0, dm=1), DTYPE, "pair"), (dict(rows=0), SHAPE, "empty"), (dict(cols=0), SHAPE, "empty"), (dict(rows=-8), SHAPE, "negative"),
    (dict(rows=2 ** 40, cols=2 ** 40, H=2 ** 38), SHAPE, "overflow"), (dict(T=3), SHAPE, "multiple of T"), (dict(B=2), SHAPE, "B * H * T"),
    (dict(H=0), SHAPE, "positive"), (dict(mbs=-1), SHAPE, "negative mask stride"), (dict(mrs=-16), SHAPE, "negative mask stride"),
    (dict(x=None), NULL, "NULL"), (dict(y=None), NULL, "NULL"),
    (dict(rows=2 ** 33, H=2 ** 31, cols=4), UNSUPPORTED, "grid"),
]
FWD = BOTH + [(dict(y=X), ARG, "in-place"), (dict(y=M), ARG, "in-place"), (dict(st=X), ARG, "in-place"), (dict(st=Y), ARG, "in-place")]
BWD = BOTH + [(dict(g=None), NULL, "NULL"), (dict(st=None), NULL, "NULL"), (dict(y=G), ARG, "in-place"), (dict(y=X), ARG, "in-place"),
              (dict(y=M), ARG, "in-place"), (dict(y=ST), ARG, "in-place")]


@pytest.mark.parametrize("kw,code,text", FWD)
def test_every_forward_refusal_comes_back_with_its_code(kw, code, text):
    rc, msg = call("fwd", **kw)
    assert rc == code and text in msg, (rc, msg)


@pytest.mark.parametrize("kw,code,text", BWD)
def test_every_backward_refusal_comes_back_with_its_code(kw, code, text):
    rc, msg = call("bwd", **kw)
    assert rc == code and text in msg, (rc, msg)


def test_the_refusals_come_in_the_headers_order_and_a_missing_mask_hides_its_dtype():
    assert call("fwd", ds=3, rows=0, x=None, y=X)[0] == DTYPE
    assert call("fwd", rows=0, x=None, y=X)[0] == SHAPE
    assert call("fwd", x=None, y=None)[0] == NULL
    assert call("fwd", y=X, rows=2 ** 33, H=2 ** 31, cols=4)[0] == ARG
    assert call("fwd", m=None, dm=3, x=None)[0] == NULL            # no mask: its dtype code is not looked at
    assert call("bwd", m=None, mbs=-1, g=None)[0] == NULL          # nor its strides


def test_a_seeded_fuzz_of_refusals_never_reaches_a_launch():
    """every call carries at least one fault, so none may return 0, and the code is that of the first faulty class in the header's order"""
    rng = random.Random(29)
    faults = {DTYPE: [dict(ds=3), dict(ds=7), dict(ds=1, dm=2)], SHAPE: [dict(rows=0), dict(T=3), dict(B=3), dict(mrs=-1), dict(cols=-2)],
              NULL: [dict(x=None)], ARG: [dict(y=X), dict(y=M)]}
    order = [DTYPE, SHAPE, NULL, ARG]
    for _ in range(200):
        picked = rng.sample(order, rng.randint(1, 4))
        kw = {}
        for c in picked:
            kw.update(rng.choice(faults[c]))
        if kw.get("y", 1) is None and ARG in picked:
            picked.remove(ARG)
        for which in ("fwd", "bwd"):
            rc, msg = call(which, **kw)
            assert rc == min(picked, key=order.index) and msg, (which, kw, rc, msg)


# ---- the Python front-end -------------------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_by_default():
    with pytest.raises(RuntimeError, match="allow_cpu_tensors"):
        attention.attn_softmax(torch.zeros(1, 1, 2, 4), None, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.attn_softmax_forward(torch.zeros(1, 1, 2, 4), None, 8)


def test_python_argument_refusals():
    x = torch.zeros(1, 2, 3, 4)
    for bad, exc in ((dict(scores=x.double()), TypeError), (dict(scores=x.bfloat16(), attention_mask=torch.zeros(1, 1, 3, 4).half()), TypeError),
                     (dict(scores=x[0]), ValueError), (dict(scores=x, attention_mask=torch.zeros(1, 2, 3, 4)), ValueError),
                     (dict(scores=x, attention_mask=torch.zeros(2, 1, 3, 4)), ValueError), (dict(scores=x[:, :0]), ValueError),
                     (dict(scores=x, head_dim=0), ValueError), (dict(scores=x, head_dim=8.0), TypeError), (dict(scores=x, head_dim=None), TypeError),
                     (dict(scores=x, head_dim=8, scale=0.1), TypeError), (dict(scores=[1.0]), TypeError)):
        kw = dict(dict(attention_mask=None, head_dim=8), **bad)
        with pytest.raises(exc):
            ops.check_attn_softmax(kw["scores"], kw["attention_mask"], kw["head_dim"], kw.get("scale"))
    with pytest.raises(ValueError, match="requires grad"):
        attention.attn_softmax(x, torch.zeros(1, 1, 3, 4, requires_grad=True), 8)
    assert ops.check_attn_softmax(x, torch.zeros(1, 1, 3, 4), 128)[:4] == (1, 2, 3, 4)


def test_inv_is_the_fp32_reciprocal_of_the_fp32_root():
    for hd in (1, 2, 3, 64, 80, 96, 128, 256):
        want = float(torch.tensor(1.0) / torch.tensor(hd ** 0.5, dtype=torch.float32))
        assert ops.attn_inv(hd) == want
    assert ops.attn_inv(scale=0.1) == float(torch.tensor(0.1, dtype=torch.float32))


def test_the_public_names_live_in_the_submodule():
    assert attention.__all__ == ["attn_softmax", "install", "convert"] and llm_qat_amd.attention is attention
    assert "attn_softmax" not in llm_qat_amd.__all__ and not hasattr(llm_qat_amd, "attn_softmax")
    assert set(ops.attn_counts) == {"fwd_launch", "bwd_launch", "copy_route"}


def test_fake_tensors_through_both_compiled_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        for ds, dm in ((torch.bfloat16, torch.float32), (torch.float16, torch.float16), (torch.float32, None)):
            x = torch.empty(2, 3, 4, 40, dtype=ds, device="cuda").transpose(1, 2).contiguous().transpose(1, 2)
            m = None if dm is None else torch.empty(2, 1, 4, 40, dtype=dm, device="cuda")
            for need in (True, False):
                y, st = compiled.attn_softmax_fwd_op(x, m, 0.125, need)
                assert y.shape == x.shape and y.dtype == ds and y.is_contiguous()
                assert st.dtype == torch.float32 and tuple(st.shape) == ((24, 2) if need else (0, 2))
            dx = compiled.attn_softmax_bwd_op(torch.empty_like(y), x, m, st, 0.125)
            assert dx.shape == x.shape and dx.dtype == ds and dx.is_contiguous()
        with pytest.raises(TypeError):
            compiled.attn_softmax_fwd_op(torch.empty(1, 1, 2, 4, dtype=torch.float64, device="cuda"), None, 0.1, True)


# ---- install / convert on a stub namespace --------------------------------------------------------------------------------------------------------------
def _stub_namespace():
    """a module object with the reference's names, written from the contract: a LlamaAttention whose forward is the eager chain"""
    import math
    ns = types.ModuleType("stub_modeling")
    src = '''
import math
import torch
from torch import nn

class Rotary(nn.Module):
    def __init__(self, dim, n=64):
        super().__init__()
        inv = 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
        emb = torch.einsum("i,j->ij", torch.arange(n).float(), inv)
        emb = torch.cat((emb, emb), -1)
        self.register_buffer("cos_cached", emb.cos()[None, None], persistent=False)
        self.register_buffer("sin_cached", emb.sin()[None, None], persistent=False)
    def forward(self, x, seq_len):
        return self.cos_cached[:, :, :seq_len].to(x.dtype), self.sin_cached[:, :, :seq_len].to(x.dtype)

def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)

def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
    cos, sin = cos[0, 0][position_ids].unsqueeze(1), sin[0, 0][position_ids].unsqueeze(1)
    return q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin

class LlamaAttention(nn.Module):
    def __init__(self, hidden=32, heads=4):
        super().__init__()
        self.hidden_size, self.num_heads, self.head_dim, self.kv_bits = hidden, heads, hidden // heads, 32
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = (nn.Linear(hidden, hidden, bias=False) for _ in range(4))
        self.rotary_emb = Rotary(self.head_dim)
    def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False):
        b, t, _ = hidden_states.shape
        sp = lambda x: x.view(b, t, self.num_heads, self.head_dim).transpose(1, 2)
        q, k, v = sp(self.q_proj(hidden_states)), sp(self.k_proj(hidden_states)), sp(self.v_proj(hidden_states))
        s = t + (past_key_value[0].shape[-2] if past_key_value is not None else 0)
        cos, sin = self.rotary_emb(v, seq_len=s)
        q, k = apply_rotary_pos_emb(q, k, cos, sin, position_ids)
        if past_key_value is not None:
            k, v = torch.cat([past_key_value[0], k], 2), torch.cat([past_key_value[1], v], 2)
        past_key_value = (k, v) if use_cache else None
        w = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(self.head_dim)
        if attention_mask is not None:
            w = torch.max(w + attention_mask, torch.tensor(torch.finfo(w.dtype).min))
        w = nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        o = torch.matmul(w, v).transpose(1, 2).reshape(b, t, self.hidden_size)
        return self.o_proj(o), (w if output_attentions else None), past_key_value
'''
    exec(compile(src, "stub_modeling", "exec"), ns.__dict__)
    return ns


def _run(m, past=False):
    torch.manual_seed(3)
    b, t, p = 2, 5, 3 if past else 0
    h = torch.randn(b, t, 32)
    neg = torch.finfo(torch.float32).min
    mask = torch.full((t, t + p), neg).triu(1 + p).expand(b, 1, t, t + p)
    pkv = tuple(torch.randn(b, 4, p, 8) for _ in range(2)) if past else None
    return m(h, attention_mask=mask, position_ids=torch.arange(p, p + t).expand(b, t), past_key_value=pkv, output_attentions=True, use_cache=True)


def test_install_and_convert_on_a_stub_namespace(cpu_route):
    ns = _stub_namespace()
    parent = ns.LlamaAttention
    torch.manual_seed(0)
    old = parent()
    with pytest.raises(TypeError):
        attention.install(object())
    assert attention.install(ns) is parent and issubclass(ns.LlamaAttention, parent) and ns.LlamaAttention is not parent
    assert ns.LlamaAttention.__name__ == "LlamaAttention"
    new = ns.LlamaAttention()
    assert list(new.state_dict()) == list(old.state_dict())
    new.load_state_dict(old.state_dict())
    for past in (False, True):
        (o0, w0, kv0), (o1, w1, kv1) = _run(old, past), _run(new, past)
        assert torch.equal(o0, o1) and torch.equal(w0, w1) and all(torch.equal(a, b) for a, b in zip(kv0, kv1))
    assert new(torch.randn(1, 2, 32), position_ids=torch.arange(2)[None])[1:] == (None, None)
    with pytest.raises(ValueError, match="Attention mask should be of size"):
        new(torch.randn(1, 2, 32), attention_mask=torch.zeros(1, 1, 2, 3), position_ids=torch.arange(2)[None])
    # the rotary function is looked up in the namespace at call time: rope.install composes, in either order
    calls = []
    eager_rot = ns.apply_rotary_pos_emb
    ns.apply_rotary_pos_emb = lambda *a: (calls.append(1), eager_rot(*a))[1]
    _run(new)
    assert calls == [1]
    ns.apply_rotary_pos_emb = eager_rot
    prev = rope.install(ns)
    assert prev is eager_rot and ns.apply_rotary_pos_emb is rope.apply_rotary_pos_emb
    assert torch.equal(_run(new)[0], _run(old)[0])                   # rope's CPU route under the opt-in: the chain's bits
    ns.apply_rotary_pos_emb = prev
    ns.LlamaAttention = parent                                       # undo
    # convert: in place, idempotent, keys unchanged, the count returned
    model = torch.nn.ModuleDict({"a": old, "b": torch.nn.Linear(2, 2), "c": torch.nn.ModuleList([parent()])})
    keys = list(model.state_dict())
    want = _run(old)
    assert attention.convert(model) == 2 and attention.convert(model) == 0
    assert model["a"] is old and isinstance(old, parent) and type(old) is not parent and type(old) is type(model["c"][0])
    assert list(model.state_dict()) == keys
    got = _run(old)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(TypeError):
        attention.convert([old])


def test_the_fused_forward_calls_attn_softmax_once_with_the_scores_and_the_head_size(cpu_route, monkeypatch):
    ns = _stub_namespace()
    attention.install(ns)
    seen = []
    real = attention.attn_softmax
    monkeypatch.setattr(attention, "attn_softmax", lambda s, m=None, hd=None, **kw: (seen.append((tuple(s.shape), hd)), real(s, m, hd, **kw))[1])
    _run(ns.LlamaAttention(), past=True)
    assert seen == [((2, 4, 5, 8), 8)]
