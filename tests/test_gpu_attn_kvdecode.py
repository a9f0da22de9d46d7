"""GPU tier of the decode attention over a codes cache (llm_qat_amd.attention.kv_decode_attention): the kernel against
the float64 chain of tests/attn_kvdecode_reference.py under section 30's cap, the three load routes bit for bit, decode_attention on the
materialised cache bit for bit, and a module that keeps its cache as codes."""
import copy
import functools
import itertools

import pytest
import torch

from llm_qat_amd import attention, ops
from llm_qat_amd.utils_quant import SymQuantizer

import attn_decode_reference as R
import attn_kvdecode_reference as KR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, FH = torch.bfloat16, torch.float16
BITS = {"int8": 8, "int4": 4}


def fused(a, mask, D, container):
    with torch.no_grad():
        return attention.kv_decode_attention(a["q"], a["k_codes"], a["k_t2"], a["v_codes"], a["v_t2"], mask, D, num_bits=BITS[container],
                                             rotary=a["rotary"], key_positions=a["key_positions"])


@functools.lru_cache(maxsize=None)
def first_split(D):
    """the first S at which the entry point cuts S into more than one chunk, for this device"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return next(S for S in range(2, 1 << 14) if ops.attn_kvdecode_workspace(R.B, R.H, 1, D, S, cus)[1] > 1)


@pytest.mark.parametrize("container,dtype,D,kind,rot", itertools.product(("int8", "int4"), (BF, FH), (64, 128), ("none", "f32"), (False, True)))
def test_every_operand_stage_is_within_the_cap(container, dtype, D, kind, rot):
    """tile edges, and both sides of the first chunk split; T walks 1, 3, 16 across them.  The largest C_out seen on the MI355X is in
    DESIGN.md section 33"""
    seen = []
    for i, S in enumerate((1, 31, 32, 33, first_split(D) - 1, first_split(D))):
        T = R.TS[i % 3]
        a = KR.inputs(T, S, D, dtype, container, DEV, rot)
        mask = R.mask_of(kind, T, S, dtype, DEV, batch=R.B if S % 2 else 1, pad=S // 4)
        seen.append((KR.measure(fused(a, mask, D, container), a, mask, D, container, dtype), T, S))
    print("kv fused C_out", container, dtype, D, kind, rot, max(seen))
    assert all(c <= R.CAP for c, _, _ in seen), seen


@pytest.mark.parametrize("container,dtype,D", [("int8", BF, 128), ("int4", FH, 64), ("int4", BF, 128), ("int8", FH, 64)])
def test_the_three_load_routes_and_decode_attention_give_the_same_bits(container, dtype, D):
    T, S = 3, first_split(D) + 5
    a = KR.inputs(T, S, D, dtype, container, DEV)
    mask = R.mask_of("f32", T, S, dtype, DEV)
    got = fused(a, mask, D, container)
    assert not a["k_codes"].is_contiguous() and torch.equal(got, fused(a, mask, D, container))
    cat = dict(a, **{n: torch.cat([a[n][:, :, :40], a[n][:, :, 40:]], 2) for n in ("k_codes", "v_codes")})      # head-major, as a grown cache
    assert cat["k_codes"].is_contiguous() and torch.equal(fused(cat, mask, D, container), got)
    off = dict(cat, **{n: torch.empty(cat[n].numel() + 1, dtype=cat[n].dtype, device=DEV)[1:].view(cat[n].shape).copy_(cat[n]) for n in ("k_codes", "v_codes")})
    assert off["k_codes"].data_ptr() % 16 and torch.equal(fused(off, mask, D, container), got)                 # the byte-load path
    # the cache materialised by QuantExport.dequantize() and ops.rope_forward, through decode_attention: the PV key order is kept, so equal bits
    B, H = R.B, R.H
    flat = {n: a[n + "_codes"].transpose(1, 2).reshape(B * S, -1) for n in "kv"}
    k, v = (ops.QuantExport(kind="sym", bins=flat[n], scales=torch.stack((a[n + "_t2"], a[n + "_t2"]), -1).reshape(B * S, 2), container=container,
                            num_bits=BITS[container], shape=(B, S, H * D), rows=B * S, cols=H * D, dtype=dtype, group_size=None).dequantize()
            .view(B, S, H, D).transpose(1, 2) for n in "kv")
    k = ops.rope_forward(k, k, *a["rotary"], a["key_positions"])[1]
    with torch.no_grad():
        assert torch.equal(attention.decode_attention(a["q"], k, v, mask, D), got)


@pytest.mark.parametrize("bits", [8, 4])
def test_a_module_keeps_its_cache_as_codes(bits):
    """a prompt of 5 tokens, then 3 single-token steps over the codes cache, against the same module with decode=True only.  Both run one
    chain on the same operands (the codes ARE the fake-quantized values; an 8-bit bf16 code may saturate at 127 where the value's is 128,
    2 u of one element), so the attention outputs differ by what a last-place flip of a score does: the cap times u max_s |v|, which
    bounds section 30's u sum_s p_s |v_s| from above"""
    from test_attn_softmax_cpu import _stub_namespace
    torch.manual_seed(11)
    base = _stub_namespace().LlamaAttention(hidden=128, heads=2).to(DEV).to(BF)
    base.kv_bits, base.act_quantizer_k, base.act_quantizer_v = bits, SymQuantizer, SymQuantizer
    base.act_clip_val_k = base.act_clip_val_v = torch.tensor([-2.0, 2.0])
    plain, codes = copy.deepcopy(base), copy.deepcopy(base)
    assert attention.convert(plain, decode=True) == 1 and attention.convert(codes, decode=True, kv_codes=True) == 1
    seen = {}
    for name, m in (("plain", plain), ("codes", codes)):
        m.o_proj.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args[0]))
    past, n, before = {"plain": None, "codes": None}, 0, dict(ops.kvdecode_counts)
    with torch.no_grad():
        for t in (5, 1, 1, 1):
            h = torch.randn(2, t, 128, device=DEV).to(BF)
            mask = torch.full((t, n + t), torch.finfo(torch.float32).min, device=DEV).triu(n + 1).expand(2, 1, t, n + t)
            for name, m in (("plain", plain), ("codes", codes)):
                past[name] = m(h, attention_mask=mask, position_ids=torch.arange(n, n + t, device=DEV).expand(2, t), past_key_value=past[name], use_cache=True)[2]
            n += t
            vmax = past["plain"][1].double().abs().amax(2).transpose(1, 2).reshape(2, 1, 128)      # max over keys of |v|, per (b, h, d) as o_proj sees it
            err = (seen["codes"].double() - seen["plain"].double()).abs() / (R.U[BF] * vmax)
            print("module C_out-style", bits, n, float(err.max()))
            assert float(err.max()) <= R.CAP
            c = past["codes"]
            assert len(c) == 5 and c[0].dtype == c[1].dtype == (torch.int8 if bits == 8 else torch.uint8) and c[0].shape[-2] == n == c[4].shape[1]
    assert ops.kvdecode_counts == dict(before, fwd_launch=before["fwd_launch"] + 3)
