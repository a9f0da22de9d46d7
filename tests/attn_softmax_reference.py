"""Reference, error measures, case list and caps for the fused attention softmax (llm_qat_amd.attention).

Torch only, no product code.  The fused kernels sum a row in another order than ATen's softmax and use the hardware exponential, so
their bar is not the chain's bits but the chain's own error: both are measured against float64 on the SAME z (the chain's value behind the
clamp, with its roundings, computed in torch ops on the tensors' device), in units of 2^-24 (fp32's unit roundoff), with u, A the one
output rounding and the flush-to-zero allowance of tests/kd_loss_reference.py (U_OUT, A_OUT):

  C_y  = max (|y - p64| - u p64 - A)+ / p64
  C_dx = max (|dx - dx64| - 2u |dx64| - 2A)+ / (inv p64 (|g| + sum_row |g p64|))       2u, 2A: the gradient is rounded to 16 bits twice,
                                                                                       and either rounding can fall into fp16's subnormals

The denominators are the magnitudes of what is multiplied, subtracted and added up, so the measures are well-conditioned where the results
cancel.  No element is left out: where p64 is 0 (a masked column), y and dx must be exactly 0.  Each cap is 4 x the eager fp32 chain's
largest measure over CASES on the MI355X: a factor 2 for the hardware exponential against ATen's, times 2 for another summation order
(the margin of sections 22 and 25).  The caps come from the eager chain, never from the kernels.
"""
import math

import torch

from kd_loss_reference import A_OUT, U_OUT, UNIT

HEAD_DIM = 128

# The eager fp32 chain's largest measures over CASES, as measured by eager_measures():
#   on the MI355X (ROCm's ATen kernels):  C_y 18.3729 (randn_s60_S33_none), C_dx 17.2965 (randn_s60_S33_causal)       <- what the caps are made of
#   on the CPU (ATen's CPU kernels):      C_y 60.0508 (ramp_S2049_none), C_dx 45.6167 (randn_s60_S2049_none)
# The fused path runs on the MI355X, so its bar is the chain it replaces there.  (The fused path itself, fp32: 27.2 and 27.4.)
# The launch ladder's cases (tests/row_ladder_cases.py: a seeded row that three elements carry, 1 .. 16392 columns) are part of the list
# since tests/test_gpu_attn_softmax_shapes.py measures the chain on each of them beside the kernels.  On the MI355X its largest measures
# there: C_y 18.9271 (520 columns, masked; 18.70 at 516, 18.54 at 512, below 18 elsewhere), C_dx 11.386 (2044 columns, masked).  C_y is
# above CASES' 18.3729, so the cap on y is made of it (73.52 -> 75.72); the cap on dx stays CASES'.  (The fused path there, fp32: 32.9, 16.4.)
EAGER_C_Y = 18.93
EAGER_C_DX = 17.30
Y_CAP = 4 * EAGER_C_Y
DX_CAP = 4 * EAGER_C_DX


def device_inv(head_dim, device):
    """what `tensor / math.sqrt(head_dim)` multiplies by: a true division on the CPU (None), the fp32 reciprocal on the GPU"""
    if torch.device(device).type == "cpu":
        return None
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(math.sqrt(head_dim), dtype=torch.float32))


def inv64(head_dim, device):
    inv = device_inv(head_dim, device)
    return 1.0 / float(torch.tensor(math.sqrt(head_dim), dtype=torch.float32)) if inv is None else inv


def chain(scores, mask, head_dim=HEAD_DIM):
    """the reference's lines behind the first product (models/modeling_llama_quant.py:352-375), q.dtype being the scores'"""
    attn = scores / math.sqrt(head_dim)
    if mask is not None:
        attn = attn + mask
        attn = torch.max(attn, torch.tensor(torch.finfo(attn.dtype).min))
    return torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32).to(scores.dtype)


def z_of(scores, mask, head_dim=HEAD_DIM):
    """the chain up to the clamp, in torch ops on the tensors' device -> (a, z): the values in front of and behind the clamp, in the
    promoted dtype (without a mask there is no clamp and z is a)"""
    with torch.no_grad():
        a = scores / math.sqrt(head_dim)
        if mask is None:
            return a, a
        a = a + mask
        return a, torch.max(a, torch.tensor(torch.finfo(a.dtype).min))


def ref64(scores, mask, g, head_dim=HEAD_DIM):
    """float64 softmax of z_of's exact values, and the gradient by float64 autograd through torch.max (which gives the tie rule), the casts
    as the identity, times inv -> dict(p, dx, g, inv): float64 tensors on the scores' device"""
    a, _ = z_of(scores, mask, head_dim)
    a64 = a.double().requires_grad_(True)
    z64 = a64 if mask is None else torch.max(a64, torch.tensor(torch.finfo(a.dtype).min, dtype=torch.float64))
    p = torch.softmax(z64, dim=-1)
    g64 = g.detach().double()
    inv = inv64(head_dim, scores.device)
    (da,) = torch.autograd.grad(p, a64, g64)
    return dict(p=p.detach(), dx=da * inv, g=g64, inv=inv, a=a64.detach(), min=None if mask is None else torch.finfo(a.dtype).min)


def recipe64(ref):
    """the contract's backward in float64, written out, from ref64's p, g, a -> dx"""
    p, g, a = ref["p"], ref["g"], ref["a"]
    d = (g - (g * p).sum(-1, keepdim=True)) * p
    if ref["min"] is not None:
        d = torch.where(a > ref["min"], d, torch.where(a == ref["min"], d / 2, torch.zeros_like(d)))
    return d * ref["inv"]


def _ratio(num, den):
    return torch.where(num == 0, torch.zeros_like(num), num / den)     # 0 / 0 where a product underflows: no error, no measure


def _excess(got, want, dtype, nu):
    u, a = U_OUT[dtype], A_OUT[dtype]
    return ((got.detach().double() - want).abs() - nu * (u * want.abs() + a)).clamp_min(0)


def c_y(y, ref):
    return float(_ratio(_excess(y, ref["p"], y.dtype, 1), ref["p"]).max() / UNIT)


def c_dx(dx, ref):
    p, g = ref["p"], ref["g"]
    den = ref["inv"] * p * (g.abs() + (g * p).abs().sum(-1, keepdim=True))
    return float(_ratio(_excess(dx, ref["dx"], dx.dtype, 2), den).max() / UNIT)


def masked_pattern(kind, T, S):
    """-> bool [1, 1, T, S], True where the mask holds finfo.min, or None.  The T rows are the last T tokens of S (a past of S - T)."""
    if kind == "none":
        return None
    col = torch.arange(S).unsqueeze(0)
    m = col > (S - T + torch.arange(T)).unsqueeze(1)          # causal
    if kind == "padded":
        m = m | (col < S // 4)                                   # left padding
    return m.reshape(1, 1, T, S)


def mask_of(pattern, dtype, device="cpu"):
    """the additive mask of a pattern: finfo(dtype).min where True, 0 elsewhere"""
    if pattern is None:
        return None
    return torch.where(pattern, torch.finfo(dtype).min, 0.0).to(dtype).to(device)


def _case(T, S, sigma, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    # bf16-representable values, so that every dtype of the GPU tier sees the inputs the caps were measured on
    x = (torch.randn((1, 1, T, S), generator=gen) * sigma).bfloat16().float()
    g = torch.randn((1, 1, T, S), generator=gen).bfloat16().float()
    return x, masked_pattern(kind, T, S), g


def cases():
    """name -> (scores fp32 [1, 1, 4, S], pattern or None, g fp32), on the CPU"""
    out = {}
    for sigma in (1.0, 8.0, 60.0):
        for S in (33, 2049, 4099):
            for kind in ("causal", "padded", "none"):
                out[f"randn_s{sigma:g}_S{S}_{kind}"] = _case(4, S, sigma, kind, int(sigma) * 10000 + S + len(kind))
    S = 2049
    ramp = (torch.arange(S, dtype=torch.float32) * 0.125).reshape(1, 1, 1, S) * torch.tensor([1.0, -1.0, 4.0, 0.5]).reshape(1, 1, 4, 1)
    out["ramp_S2049_none"] = (ramp.bfloat16().float(), None, _case(4, S, 1.0, "none", 77)[2])
    return out


_CASES = None


def CASES():
    """the case list, built once and shared; callers leave the tensors unchanged"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def eager32(scores, mask, g, head_dim=HEAD_DIM):
    """the chain and its autograd gradient -> y, dx"""
    x = scores.detach().requires_grad_(True)
    y = chain(x, mask, head_dim)
    (dx,) = torch.autograd.grad(y, x, g)
    return y.detach(), dx


def eager_measures(device="cpu"):
    """name -> (C_y, C_dx) of the eager fp32 chain on `device`: what the caps are made of"""
    out = {}
    for name, (x, pattern, g) in CASES().items():
        x, g, mask = x.to(device), g.to(device), mask_of(pattern, torch.float32, device)
        ref = ref64(x, mask, g)
        y, dx = eager32(x, mask, g)
        out[name] = (c_y(y, ref), c_dx(dx, ref))
    return out
