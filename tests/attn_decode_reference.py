"""Reference, error measure, case list and cap for the fused decode attention (llm_qat_amd.attention.decode_attention).

Torch only.  The chain in float64 from the exact 16-bit inputs with the roundings in front of the softmax kept: x = the first product
rounded to the dtype, x * inv rounded to the dtype (inv: the fp32 reciprocal of the fp32 root), the sum with the mask in the promoted
dtype, the clamp under a mask only.  q and k are multiples of 1/4 in [-2, 2]: every partial sum of a product row is a multiple of 1/16
below 2^10, exact in fp32 in any order, so x is one number for the reference, the library GEMM and the kernel, and no rounding of x can
fall the other way (one unit of x's last place in z, which no bound on `out` could absorb).

  C_out = max over (t, d) of |out - ref64| / (u sum_s p_s |v_s,d|),      u_bf16 = 2^-8, u_fp16 = 2^-11

The cap is 4 x the composed path's (matmul, attn_softmax, matmul) largest C_out over the case list on the MI355X: section 29's factor.
"""
import functools
import itertools

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
S_FIXED = (1, 15, 16, 17, 31, 32, 33, 4099)
S_MAX = max(S_FIXED)
TS = (1, 3, 16)
DIMS = list(itertools.product((64, 128), (torch.bfloat16, torch.float16), ("none", "ds", "f32")))
B, H = 2, 3

# Largest C_out over DIMS x TS x key_counts (S_FIXED and both sides of all 69 chunk-count changes up to 4099 for B * H = 6 on 256 compute
# units) on the MI355X, by tools/attn_decode_bench.py --measure:
#   the composed path:  1.9505 (D 128, bf16, fp32 mask, T 3, S 2721)       <- what the cap is made of: 4 x 1.95 = 7.80
#   the fused kernel:   1.5735 (D 128, bf16, masked, T 16, S 16)            beside it, never part of the cap
COMPOSED_C_OUT = 1.95
CAP = 4 * COMPOSED_C_OUT


def inv_of(D):
    return float(torch.tensor(1.0) / torch.tensor(D ** 0.5, dtype=torch.float32))


def key_counts(nsplit_of):
    """S_FIXED, and one S below and one at EVERY change of the chunk count up to S_MAX; nsplit_of(S): the entry point's own answer"""
    n = [nsplit_of(S) for S in range(1, S_MAX + 1)]
    return sorted(set(S_FIXED) | {s for S in range(2, S_MAX + 1) if n[S - 1] != n[S - 2] for s in (S - 1, S)})


@functools.lru_cache(maxsize=None)
def _pool(D, dtype, device, seed, B, H, n):
    g = torch.Generator().manual_seed(seed * 100003 + D)
    q, k = (torch.randint(-8, 9, (B, H, n, D), generator=g).float() / 4 for n in (max(TS), n))
    return q.to(dtype).to(device), k.to(dtype).to(device), torch.randn((B, H, k.shape[2], D), generator=g).to(dtype).to(device)


def inputs(T, S, D, dtype, device, seed=0, signed_v=False, B=B, H=H, pool=S_MAX):
    """q [B, H, T, D], k, v [B, H, S, D]: the leading rows of one seeded pool per (D, dtype).  Query row 0 is seeded: its largest score is
    at key 0, the second at the last key, the third at the middle key, and v is largest there too, so a first, middle or last chunk or
    tile that is dropped or counted twice shows in row 0.  Query row 1 (where T > 1) is zero: a uniform softmax over whatever the mask
    leaves, whose result moves by one tile's share of the keys if any tile is lost, which fp16 resolves up to some hundred tiles."""
    q, k, v = (t[:, :, :n].clone() for t, n in zip(_pool(D, dtype, device, seed, B, H, pool), (T, S, S)))
    v = v if signed_v else v.abs() + 0.25
    q[:, :, 0] = 2.0
    q[:, :, 1:2] = 0.0
    for i, (key, zeros) in reversed(list(enumerate(((0, 0), (S - 1, 3), (S // 2, 6))))):      # where S is short and keys coincide, the earlier wins
        k[:, :, key] = 2.0
        k[:, :, key, :zeros] = 0.0
        v[:, :, key] = 4.0 * 2 ** i
    return q, k, v


def mask_of(kind, T, S, dtype, device, batch=B, pad=0):
    """None, or the additive causal-with-past mask [batch, 1, T, S] (the T rows are the last T tokens of S) with finfo.min where masked;
    pad > 0: the first `pad` keys of the last batch element are masked too (left padding)"""
    if kind == "none":
        return None
    mdt = dtype if kind == "ds" else torch.float32
    col = torch.arange(S, device=device)
    m = (col[None] > (S - T + torch.arange(T, device=device))[:, None]).expand(batch, 1, T, S).clone()
    m[-1] |= col < pad
    return torch.where(m, torch.finfo(mdt).min, 0.0).to(mdt)


def ref64(q, k, v, mask, inv):
    """-> (out, mag): the chain in float64 and sum_s p_s |v_s,d|, both [B, H, T, D] float64 on q's device"""
    x = (q.double() @ k.double().transpose(2, 3)).to(q.dtype)
    z = (x.float() * inv).to(q.dtype)
    if mask is not None:
        P = torch.promote_types(q.dtype, mask.dtype)
        z = torch.max(z.to(P) + mask.to(P), torch.tensor(torch.finfo(P).min, dtype=P, device=q.device))
    p = torch.softmax(z.double(), -1)
    return p @ v.double(), p @ v.double().abs()


def c_out(out, ref, mag):
    return float(((out.double() - ref).abs() / (U[out.dtype] * mag)).max())
