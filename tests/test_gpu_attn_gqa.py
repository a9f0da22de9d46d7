"""Grouped-query attention in the decode, codes-cache and prefill kernels against the float64 chain over the
expanded k, v, under the ungrouped kernels' caps (the arithmetic of a query row is unchanged), and against the ungrouped call's bits
where both cut S into one chunk.  Inputs, references and caps are the ungrouped kernels' modules'."""
import pytest
import torch

import attn_decode_reference as R
import attn_kvdecode_reference as K
import attn_prefill_reference as P
from llm_qat_amd import attention, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, HKV = 2, 2
# (G, T): four live columns; two full packs; 12 live columns; 15 columns with an odd G; HP = 5 in two packs, the second partial; HP = 1
GT = [(4, 1), (4, 4), (8, 2), (4, 3), (3, 5), (8, 3), (2, 16)]
S_DECODE = (1, 33, 224, 225, 1025)      # 224: the last S of one chunk, 225: two, 1025: several
S_CODES = (33, 224, 225)
DIMS = [(D, dt) for D in (64, 128) for dt in (torch.bfloat16, torch.float16)]
ONE_CHUNK = 224


def expand(t, G):
    return t.repeat_interleave(G, 1)


def mask_of(masked, T, S, dtype):
    """None, or the fp32 causal-with-past mask with left padding; batch stride 0 at even S"""
    return R.mask_of("f32", T, S, dtype, DEV, batch=B if S % 2 else 1, pad=S // 4) if masked else None


def heads_differ(ref, mag, G, dtype):
    """on the float64 reference: any two heads of a group differ somewhere by more than the cap's error, so a wrong head map cannot pass"""
    r, bound = ref.unflatten(1, (HKV, G)), (R.CAP * R.U[dtype] * mag).unflatten(1, (HKV, G))
    return all(bool(((r[:, :, a] - r[:, :, b]).abs() > torch.maximum(bound[:, :, a], bound[:, :, b])).any()) for a in range(G) for b in range(a))


def decode_inputs(G, T, S, D, dtype):
    """R.inputs with H = HKV G query heads and the first HKV heads of k, v.  Row 0 is 2.0 in every head there: at T = 1 the heads of a
    group would agree and a wrong head map would pass.  The first head of each group keeps that seeded row; the others are lowered by a
    seeded multiple of 1/4 per element (values in [-2, 2], every product still exact).  One offset per head is not enough: where the
    mask leaves one seeded key, every positive row 0 saturates the softmax on it and the heads agree within the cap"""
    q, k, v = R.inputs(T, S, D, dtype, DEV, B=B, H=HKV * G, pool=max(S_DECODE))
    off = 0.25 * torch.randint(0, 17, (HKV * G, D), generator=torch.Generator().manual_seed(G)).float()
    off[::G] = 0.0
    q[:, :, 0] = (2.0 - off).to(dtype).to(DEV)
    return q, k[:, :HKV].contiguous(), v[:, :HKV].contiguous()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "f32mask"])
@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("G,T", GT)
def test_decode(G, T, D, dtype, masked):
    for S in S_DECODE:
        q, k, v = decode_inputs(G, T, S, D, dtype)
        mask = mask_of(masked, T, S, dtype)
        ref, mag = R.ref64(q, expand(k, G), expand(v, G), mask, R.inv_of(D))
        assert S == 1 or heads_differ(ref, mag, G, dtype), (S, "the heads of a group must differ")      # S = 1: out is v[0] whatever q is
        out = attention.decode_attention(q, k, v, mask, D)
        c = R.c_out(out, ref, mag)
        print(f"decode G={G} T={T} S={S} D={D} {dtype} masked={masked}: C_out {c:.4f}")
        assert c <= R.CAP, (S, c)
        assert torch.equal(out, attention.decode_attention(q, k, v, mask, D)), (S, "two calls differ")
        if S <= ONE_CHUNK:
            assert torch.equal(out, attention.decode_attention(q, expand(k, G), expand(v, G), mask, D)), (S, "not the expanded call's bits")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "f32mask"])
@pytest.mark.parametrize("rot", [False, True], ids=["norot", "rot"])
@pytest.mark.parametrize("container", ["int8", "int4"])
@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("G,T", GT)
def test_codes_cache(monkeypatch, G, T, D, dtype, container, rot, masked):
    monkeypatch.setattr(K, "H", HKV * G)      # K.inputs' head count: q of H heads, of whose codes the first HKV are the cache
    bits = 8 if container == "int8" else 4
    for S in S_CODES:
        a = K.inputs(T, S, D, dtype, container, DEV, rot=rot)
        a["k_codes"], a["v_codes"] = a["k_codes"][:, :HKV], a["v_codes"][:, :HKV]      # views of the export layout, head stride D
        wide = dict(a, k_codes=expand(a["k_codes"], G), v_codes=expand(a["v_codes"], G))
        mask = mask_of(masked, T, S, dtype)
        k, v = K.operands(wide["k_codes"], a["k_t2"], wide["v_codes"], a["v_t2"], container, dtype, a["rotary"], a["key_positions"])
        assert heads_differ(*R.ref64(a["q"], k, v, mask, R.inv_of(D)), G, dtype), (S, "the heads of a group must differ")

        def call(x):
            return attention.kv_decode_attention(x["q"], x["k_codes"], x["k_t2"], x["v_codes"], x["v_t2"], mask, D, num_bits=bits, rotary=x["rotary"],
                                                 key_positions=x["key_positions"])
        out = call(a)
        c = K.measure(out, wide, mask, D, container, dtype)
        print(f"codes G={G} T={T} S={S} D={D} {dtype} {container} rot={rot} masked={masked}: C_out {c:.4f}")
        assert c <= R.CAP, (S, c)
        assert torch.equal(out, call(a)), (S, "two calls differ")
        if S <= ONE_CHUNK:
            assert torch.equal(out, call(wide)), (S, "not the expanded call's bits")


def prefill_inputs(G, T, S, D, dtype):
    """P.inputs' q of several seeds side by side as the H = HKV G query heads; k, v: the first HKV heads of seed 0"""
    parts = [P.inputs(T, S, D, dtype, DEV, seed=s) for s in range(-(-HKV * G // P.H))]
    return torch.cat([p[0] for p in parts], 1)[:, :HKV * G].contiguous(), parts[0][1][:, :HKV].contiguous(), parts[0][2][:, :HKV].contiguous()


@pytest.mark.parametrize("kind", ["f32", "causal"])
@pytest.mark.parametrize("D,dtype", DIMS, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("G", [2, 4])
def test_prefill(G, D, dtype, kind):
    for T in (17, 129):
        for S in (T, T + 33):
            q, k, v = prefill_inputs(G, T, S, D, dtype)
            mask = None if kind == "causal" else mask_of(True, T, S, dtype)
            ref_mask = R.mask_of("ds", T, S, dtype, DEV) if kind == "causal" else mask
            ref, mag = P.ref64(q, expand(k, G), expand(v, G), ref_mask, P.inv_of(D))
            assert heads_differ(ref, mag, G, dtype), (T, S)
            out = attention.prefill_attention(q, k, v, mask, D, causal=kind == "causal")
            c = P.c_out(out, ref, mag)
            print(f"prefill G={G} T={T} S={S} D={D} {dtype} {kind}: C_out {c:.4f}")
            assert c <= P.CAP, (T, S, c)
            assert torch.equal(out, attention.prefill_attention(q, expand(k, G), expand(v, G), mask, D, causal=kind == "causal")), (T, S)


def misaligned(t):
    """a copy of t one element off 16-byte alignment: the byte-load path"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("kernel", ["decode", "codes", "prefill"])
def test_layouts(monkeypatch, kernel):
    """k, v as the transposed view of a [B, S, HKV D] projection and a misaligned copy give the contiguous call's bits"""
    G, T, S, D, dtype = 4, (3 if kernel != "prefill" else 17), 225, 128, torch.bfloat16
    if kernel == "codes":
        monkeypatch.setattr(K, "H", HKV * G)
        a = K.inputs(T, S, D, dtype, "int8", DEV, rot=True)
        q, k, v = a["q"], a["k_codes"][:, :HKV], a["v_codes"][:, :HKV]

        def call(q, k, v):
            return attention.kv_decode_attention(q, k, a["k_t2"], v, a["v_t2"], None, D, rotary=a["rotary"], key_positions=a["key_positions"])
    else:
        q, k, v = decode_inputs(G, T, S, D, dtype) if kernel == "decode" else prefill_inputs(G, T, S, D, dtype)
        fn = attention.decode_attention if kernel == "decode" else attention.prefill_attention

        def call(q, k, v):
            return fn(q, k, v, None, D)
    want = call(q, k.contiguous(), v.contiguous())
    proj = [t.transpose(1, 2).reshape(B, S, HKV * D).contiguous().view(B, S, HKV, D).transpose(1, 2) for t in (k, v)]
    assert not proj[0].is_contiguous() and torch.equal(call(q, *proj), want)
    assert torch.equal(call(misaligned(q), misaligned(k.contiguous()), misaligned(v.contiguous())), want)


def test_train_refuses_grouped_heads():
    q, k, v = prefill_inputs(2, 17, 17, 64, torch.bfloat16)
    with pytest.raises(ValueError, match="grouped-query"):
        attention.train_attention(q, k, v, None, 64)
