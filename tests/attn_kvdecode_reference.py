"""Inputs and reference for the decode attention over a codes cache (llm_qat_amd.attention.kv_decode_attention).

Torch only.  The cache is dequantized and rotated here in float64 with the chain's roundings (.to(ds) where QuantExport.dequantize() and
fq_rope.h's rope_fwd round), then tests/attn_decode_reference.py's float64 attention and its C_out measure take over, under that module's
cap.  The inputs keep the first product exact: codes over the container's full range, t2 a power of two per token, q in multiples of 1/4,
table entries from {0, +-1/2, +-1}, so every product q[d] khat[d] is a multiple of 2^-12 and a row's sum of magnitudes stays below 2^12:
24 bits, exact in fp32 in ANY order of d.  The kernel's permuted d order can therefore not move a rounding of x; inputs() asserts it."""
import torch

import attn_decode_reference as R

B, H = R.B, R.H


def unpack(codes, container):
    """the codes as int64 [..., D]"""
    if container == "int8":
        return codes.long()
    v = torch.stack((codes & 0xF, codes >> 4), -1).flatten(-2).long()
    return torch.where(v >= 8, v - 16, v)


def operands(k_codes, k_t2, v_codes, v_t2, container, dtype, rotary=None, key_positions=None):
    """-> (khat rotated, vhat) in `dtype`: rb(code / t2) with the fp32 quotient, k through rope_fwd's four roundings"""
    k, v = ((unpack(c, container).float() / t2[:, None, :, None]).to(dtype) for c, t2 in ((k_codes, k_t2), (v_codes, v_t2)))
    if rotary is not None:
        D, S = k.shape[-1], k.shape[2]
        pos = torch.arange(S, device=k.device)[None] if key_positions is None else key_positions
        cos, sin = (t.reshape(-1, D).to(dtype)[pos].unsqueeze(1).double() for t in rotary)
        x = k.double()
        half = torch.cat((-x[..., D // 2:], x[..., :D // 2]), -1)
        k = ((x * cos).to(dtype).double() + (half * sin).to(dtype).double()).to(dtype)
    return k, v


def inputs(T, S, D, dtype, container, device, rot=True, seed=0):
    """-> dict(q, k_codes, k_t2, v_codes, v_t2, rotary, key_positions): the codes as the [B, H, S, D] view of export-layout [B, S, H * D] bins"""
    g = torch.Generator().manual_seed(seed * 7919 + S * 31 + D)
    lo, hi, base = (-128, 128, 64.0) if container == "int8" else (-8, 8, 4.0)
    q = (torch.randint(-8, 9, (B, H, T, D), generator=g).float() / 4).to(dtype)
    out = dict(q=q)
    for name in "kv":
        c = torch.randint(lo, hi, (B, S, H, D), generator=g)
        if container == "int8":
            c = c.to(torch.int8)
        else:
            c = ((c[..., 0::2] & 0xF) | ((c[..., 1::2] & 0xF) << 4)).to(torch.uint8)
        out[name + "_codes"] = c.transpose(1, 2)
        out[name + "_t2"] = base * 2.0 ** torch.randint(-1, 2, (B, S), generator=g).float()
    out["rotary"] = out["key_positions"] = None
    if rot:
        vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0])
        out["rotary"] = tuple(vals[torch.randint(0, 5, (S, D), generator=g)].to(dtype) for _ in range(2))
        out["key_positions"] = torch.stack([torch.randperm(S, generator=g) for _ in range(B if S % 2 else 1)])      # both batch strides
    out = {n: (tuple(x.to(device) for x in t) if isinstance(t, tuple) else t.to(device) if t is not None else None) for n, t in out.items()}
    k, _ = operands(out["k_codes"], out["k_t2"], out["v_codes"], out["v_t2"], container, dtype, out["rotary"], out["key_positions"])
    prod = out["q"].double()[:, :, :, None, :] * k.double()[:, :, None, :, :]
    assert bool((prod * 4096 == (prod * 4096).round()).all()) and float(prod.abs().sum(-1).max()) < 4096, "the first product is not exact in fp32"
    return out


def measure(out, a, mask, D, container, dtype):
    """C_out of `out` against the float64 chain over the dequantized, rotated cache"""
    k, v = operands(a["k_codes"], a["k_t2"], a["v_codes"], a["v_t2"], container, dtype, a["rotary"], a["key_positions"])
    ref, mag = R.ref64(a["q"], k, v, mask, R.inv_of(D))
    exact = (mag == 0) & (out.double() == ref)      # a column whose every weighted code is 0 (S = 1, code 0): the bound is 0, met exactly
    return R.c_out(out, ref, torch.where(exact, 1.0, mag))
