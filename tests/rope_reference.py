"""Reference, formula model and case list for the fused rotary embedding (llm_qat_amd.rope).

The op has no reduction, so its bar is the eager chain's bits, with no share of elements left out: chain() is the reference's
apply_rotary_pos_emb in this project's own words (as tests/tiny_llama.py writes it, with the gather by position_ids and the cast of the
tables in front of it), chain_grads() its autograd; model_fwd / model_bwd restate the contract of include/llmqat_fakequant_rope.h in
torch fp32 ops, one rounding per line.
"""
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def tables(P, D, dtype=torch.float32, device="cpu", base=10000.0, equal_halves=True):
    """cos, sin [P, D] as the rotary module caches them (fp32, both halves equal), or with unequal halves"""
    inv = 1.0 / (base ** (torch.arange(0, D, 2, device=device).float() / D))
    ang = torch.einsum("i,j->ij", torch.arange(P, device=device, dtype=inv.dtype), inv)
    emb = torch.cat((ang, ang if equal_halves else ang * 1.37 + 0.21), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def chain(q, k, cos, sin, position_ids=None):
    """the eager chain: the tables cast to the tensors' dtype (float32 where q and k differ: the reference casts to v's dtype, which is
    k's), gathered by position, and x * cos + rotate_half(x) * sin for q and k"""
    D = q.shape[-1]
    dt = q.dtype if q.dtype == k.dtype else torch.float32
    cos, sin = cos.reshape(-1, D).to(dtype=dt), sin.reshape(-1, D).to(dtype=dt)
    if position_ids is None:
        position_ids = torch.arange(q.shape[2], device=q.device).unsqueeze(0)
    cos, sin = cos[position_ids].unsqueeze(1), sin[position_ids].unsqueeze(1)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def chain_grads(q, k, cos, sin, position_ids, gq, gk):
    """-> q_embed, k_embed, dq, dk of the chain and its autograd (q and k are taken as leaves where they lie)"""
    qr, kr = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
    qe, ke = chain(qr, kr, cos, sin, position_ids)
    dq, dk = torch.autograd.grad((qe, ke), (qr, kr), (gq, gk))
    return qe.detach(), ke.detach(), dq, dk


def _rb(t, dtype):
    return t.to(dtype).float()


def _rows(x, cos, sin, position_ids):
    """the table rows of every token, rounded to x's dtype, as fp32 [B or 1, 1, T, D]; a position outside [-P, P) gives NaN rows"""
    D, T, P = x.shape[-1], x.shape[2], cos.shape[-2]
    cos, sin = _rb(cos.reshape(-1, D), x.dtype), _rb(sin.reshape(-1, D), x.dtype)      # (the identity for the fp32 x of the two-dtype case)
    pos = torch.arange(T, device=x.device).unsqueeze(0) if position_ids is None else position_ids
    pos = torch.where(pos < 0, pos + P, pos)
    bad = (pos < 0) | (pos >= P)
    safe = pos.clamp(0, P - 1)
    nan = torch.full((), float("nan"), device=x.device)
    c = torch.where(bad.unsqueeze(-1), nan, cos[safe]).unsqueeze(1)
    s = torch.where(bad.unsqueeze(-1), nan, sin[safe]).unsqueeze(1)
    return c, s


def model_fwd(x, cos, sin, position_ids=None):
    """the contract's forward for one tensor, contiguous"""
    dt, h = x.dtype, x.shape[-1] // 2
    c, s = _rows(x, cos, sin, position_ids)
    xf = x.float()
    x1, x2 = xf[..., :h], xf[..., h:]
    y1 = _rb(x1 * c[..., :h], dt) + _rb((-x2) * s[..., :h], dt)
    y2 = _rb(x2 * c[..., h:], dt) + _rb(x1 * s[..., h:], dt)
    return torch.cat((y1, y2), dim=-1).to(dt)


def model_bwd(g, cos, sin, position_ids=None, dtype=None):
    """the contract's backward for one tensor, contiguous.  dtype: the tensor's where it is not the gradient's (q and k in two dtypes: g
    is fp32, the tables are unrounded, the roundings and the result are the 16-bit tensor's)"""
    dt, h = dtype or g.dtype, g.shape[-1] // 2
    c, s = _rows(g, cos, sin, position_ids)
    gf = g.float()
    a, b = _rb(gf * c, dt), _rb(gf * s, dt)
    d1 = _rb(a[..., :h] + b[..., h:], dt) + 0.0
    d2 = _rb(a[..., h:] + (-b[..., :h]), dt) + 0.0
    return torch.cat((d1, d2), dim=-1).to(dt)


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN (the chain's NaN payloads are ATen's business)"""
    a, b = a.detach(), b.detach()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = a.isnan()
    return bool((nan == b.isnan()).all()) and torch.equal(bits(torch.where(nan, torch.zeros_like(a), a)), bits(torch.where(nan, torch.zeros_like(b), b)))


def transposed(B, H, T, D, dtype, device, gen, scale=1.0):
    """a [B, H, T, D] tensor as the reference's attention makes it: the transposed view over [B, T, H * D] memory"""
    return (torch.randn(B, T, H * D, generator=gen) * scale).to(dtype).to(device).view(B, T, H, D).transpose(1, 2)


# the shared shapes of the GPU tier (B, Hq, Hk, T, D): D = 2 and 6 take the element path (6: three groups of a head, which do not divide the
# workgroup), 16 is the smallest fp32 vector half, 64 and 128 the real heads, 256 the widest; H = 32 at D = 128 is two sweeps of a workgroup
SHAPES = [(1, 1, 1, 1, 2), (2, 3, 1, 5, 6), (1, 3, 3, 33, 16), (2, 8, 2, 5, 64), (1, 32, 32, 5, 128), (2, 1, 3, 33, 256), (1, 3, 1, 1, 128), (2, 32, 8, 33, 64)]
