"""Float64 reference, error measures, case list and caps for the fused training attention (llm_qat_amd.attention.train_attention,
DESIGN.md section 32).  Torch only.  Inputs, masks and the case arguments are attn_prefill_reference's.

The reference.  The values in front of the softmax are the rounded chain's (x = the first product rounded to the dtype, x inv rounded
to the dtype, the sum with the mask in the promoted dtype, the clamp under a mask only); the derivative is the unrounded formula's,
written out (no autograd through 16-bit casts: that would round the reference's own gradient): p = softmax(z), g = dO v^T,
d = (g - sum_s p g) p c with c = torch.max's gradient at the clamp (1 above finfo.min, 1/2 at it, 0 below), ds = d inv, dq = ds k,
dk = ds^T q, dv = p^T dO.

The measures, in units of the dtype's u like C_out, with w = c p (|g| + sum_s' p |g|) inv:
  C_dv = max |dv - dv64| / (u sum_t p |dO|)      C_dq = max |dq - dq64| / (u sum_s w |k_s|)      C_dk = max |dk - dk64| / (u sum_t w |q_t|)
fp16 only: p and ds are stored in 16 bits in front of the second and third products on either path, and below 2^-14 such a value carries
an absolute error of up to 2^-25 whatever its size; it counts twice, as u does (section 29's trap 8), once more for the output's own
rounding: the denominators gain 2^-24 (sum_t |dO| + 1), 2^-24 (sum_s |k| + 1) and 2^-24 (sum_t |q| + 1), for both paths alike.

Each cap is 4 x the composed path's (matmul, attn_softmax, matmul under autograd) largest measure over DIMS x cases() on the MI355X, by
tools/attn_train_bench.py --measure, which rewrites the block between the two marker lines below; the fused kernels' values stand beside
them for the record and are never part of a cap."""
import functools
import itertools

import torch

from attn_prefill_reference import B, H, U, case_args, inputs, inv_of, mask_of  # noqa: F401
from llm_qat_amd import ops

DIMS = list(itertools.product((64, 128), (torch.bfloat16, torch.float16), ("none", "ds", "f32", "causal")))
QTS = sorted({ops.PREFILL_QT, ops.TRAIN_DQ_QT, ops.TRAIN_DKV_QT})      # the query tiles of the three kernels
KTS = sorted({ops.PREFILL_KT, ops.TRAIN_DQ_KT, ops.TRAIN_DKV_KT})      # and their key tiles
TS = sorted({1, 17} | {t + i for t in QTS for i in (0, 1)})
NAMES = ("out", "dq", "dk", "dv")
A16 = 2.0 ** -24

# -- measured (tools/attn_train_bench.py --measure) --
COMPOSED = {"out": 1.8106, "dq": 1.8938, "dk": 2.2554, "dv": 1.8506}
#   C_out: the composed path 1.8106 (D 128, bfloat16, f32, T 32, S 97); the fused kernels 1.6568 (D 64, bfloat16, f32, T 17, S 17), never part of the cap
#   C_dq: the composed path 1.8938 (D 128, bfloat16, f32, T 129, S 160); the fused kernels 1.3050 (D 128, bfloat16, f32, T 129, S 160), never part of the cap
#   C_dk: the composed path 2.2553 (D 128, float16, f32, T 32, S 32); the fused kernels 1.7344 (D 128, bfloat16, causal, T 32, S 97), never part of the cap
#   C_dv: the composed path 1.8506 (D 128, bfloat16, f32, T 33, S 64); the fused kernels 1.8506 (D 128, bfloat16, f32, T 33, S 64), never part of the cap
# -- end measured --
CAPS = {n: None if c is None else 4 * c for n, c in COMPOSED.items()}


def cases(kind):
    """(T, S): every query-tile boundary of the three kernels against every key-tile boundary, and one S < T where no causal rule forbids it"""
    out = [(T, T + d) for T in TS for d in sorted({0} | {kt + i for kt in KTS for i in (-1, 1)})]
    return out + ([] if kind == "causal" else [(max(QTS) + 1, min(KTS) + 1)])


@functools.lru_cache(maxsize=None)
def _dout_pool(D, dtype, device):
    return torch.randn((B, H, max(TS), D), generator=torch.Generator().manual_seed(977 + D))


def dout_of(T, D, dtype, device):
    """the upstream gradient [B, H, T, D]: signed, seeded, large at query row 0 and at the first row of the last query tile"""
    d = _dout_pool(D, dtype, device)[:, :, :T].clone()
    d[:, :, 0] *= 8.0
    d[:, :, (T - 1) // max(QTS) * max(QTS)] *= 8.0
    return d.to(dtype).to(device)


def ref64(q, k, v, mask, inv, dout):
    """-> {name: (value, magnitude)} for out, dq, dk, dv and {"m", "l"}: the row maxima and sums of exp(z - m), all float64 on q's device"""
    x = (q.double() @ k.double().transpose(2, 3)).to(q.dtype)
    z = (x.float() * inv).to(q.dtype)
    c = 1.0
    if mask is not None:
        P = torch.promote_types(q.dtype, mask.dtype)
        a, mn = z.to(P) + mask.to(P), torch.finfo(P).min
        c = torch.where(a > mn, 1.0, torch.where(a == mn, 0.5, 0.0)).double()
        z = torch.max(a, torch.tensor(mn, dtype=P, device=q.device))
    z = z.double()
    m = z.max(-1, keepdim=True).values
    e = torch.exp(z - m)
    p = e / e.sum(-1, keepdim=True)
    qd, kd, vd, gd = q.double(), k.double(), v.double(), dout.double()
    g = gd @ vd.transpose(2, 3)
    ds = (g - (g * p).sum(-1, keepdim=True)) * p * c * inv
    w = c * p * (g.abs() + (p * g.abs()).sum(-1, keepdim=True)) * inv
    a16 = A16 if q.dtype == torch.float16 else 0.0
    u = U[q.dtype]
    return {"out": (p @ vd, u * (p @ vd.abs())),
            "dq": (ds @ kd, u * (w @ kd.abs()) + a16 * (kd.abs().sum(2, keepdim=True) + 1)),
            "dk": (ds.transpose(2, 3) @ qd, u * (w.transpose(2, 3) @ qd.abs()) + a16 * (qd.abs().sum(2, keepdim=True) + 1)),
            "dv": (p.transpose(2, 3) @ gd, u * (p.transpose(2, 3) @ gd.abs()) + a16 * (gd.abs().sum(2, keepdim=True) + 1)),
            "m": m.squeeze(-1), "l": e.sum(-1)}


def measures(got, ref):
    """{name: C_name} of got = {name: tensor [B, H, T | S, D]}; an element that must be exactly 0 and is measures 0"""
    out = {}
    for n in NAMES:
        diff, (_, mag) = (got[n].double() - ref[n][0]).abs(), ref[n]
        out[n] = float(torch.where(diff == 0, 0.0, diff / mag).max())
    return out


def composed(q, k, v, mask, D, dout):
    """the path the cap is made of: matmul, attn_softmax, matmul under autograd -> {name: tensor}"""
    from llm_qat_amd import attention
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = torch.matmul(attention.attn_softmax(torch.matmul(q, k.transpose(2, 3)), mask, D), v)
    out.backward(dout)
    return {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def fused(q, k, v, mask, D, dout, causal=False):
    from llm_qat_amd import attention
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = attention.train_attention(q, k, v, mask, D, causal=causal)
    out.backward(dout)
    return {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
