"""CPU tensors (opt-in): the reference accepts tensors on any device (models/utils_quant.py:37), and BASELINE configs[0] is a
tiny-LLaMA QAT step on CPU.  This module serves CPU tensors -- and nothing else -- with plain torch ops in the reference's op order
(:50-72, :110-147, :83-87, :203-238), so that the drop-in classes run where no GPU exists.

It is NOT a fallback: it is selected by `tensor.device.type == "cpu"` only, and only after `llm_qat_amd.allow_cpu_tensors(True)` /
LLMQAT_AMD_CPU_TENSORS=1 (the default keeps raising).  A CUDA tensor never comes here: if the HIP library is missing or a launch
fails, the GPU path raises.  Nothing here touches the test infrastructure; ATen's CPU kernels ARE the reference's CPU path.
"""
import math
import os

import torch

ENABLED = os.environ.get("LLMQAT_AMD_CPU_TENSORS", "0") == "1"


def allow_cpu_tensors(flag=True):
    global ENABLED
    ENABLED = bool(flag)


def refuse(x, what):
    raise RuntimeError(f"{what}: tensor is on '{x.device}'. llm_qat_amd runs on MI355X and has no CPU fallback; move the tensor to the GPU. "
                       "(CPU tensors are served, with plain torch ops, only after llm_qat_amd.allow_cpu_tensors(True) / LLMQAT_AMD_CPU_TENSORS=1.)")


def _stat(x, layerwise, largest):
    """The statistic one scale is made of, KEPT SMALL: shape [..., 1] (ndim <= 3), [d0, d1, 1, 1] (4-D) or 0-dim (layerwise), and left to
    broadcast in the elementwise ops that follow.  The reference expands it to the input's shape first (:57, :67, :118-140); every element
    then sees the same scalar operands either way, so the values are the same bit for bit, and the per-row part of the chain runs on
    rows instead of on elements (what tests/test_cpu_tensors.py checks against the reference's own fixtures)."""
    pick = torch.max if largest else torch.min
    if layerwise:
        return pick(x)                                   # :51 / :111-112
    if x.dim() <= 3:
        return pick(x, dim=-1, keepdim=True)[0]          # :56 / :116-118
    if x.dim() == 4:
        return pick(x.view(x.shape[0], x.shape[1], -1), dim=-1, keepdim=True)[0].unsqueeze(-1)   # :63-66 / :127-139
    raise ValueError(f"fake-quant expects at most 4 dimensions, got {x.dim()}")   # :70


def forward(kind, x, num_bits, layerwise):
    if kind == "sym":
        s = (2 ** (num_bits - 1) - 1) / (_stat(torch.abs(x), layerwise, True) + 1e-6)    # int / Tensor: reciprocal() * int, per row
        return torch.round(x * s).div(s + 1e-6)                                          # :72
    beta = _stat(x, layerwise, False)
    span = (_stat(x, layerwise, True) - beta) + 1e-8                                     # alpha + 1e-8, used twice (:144, :147)
    levels = 2 ** num_bits - 1
    return torch.round((x - beta) / span * levels).div(levels) * span + beta


def backward(grad_output, x, clip_val):
    gx = grad_output.clone()
    gx[x.ge(clip_val[1])] = 0
    gx[x.le(clip_val[0])] = 0
    return gx


def low_bit_weight(w, w_bits, layerwise):
    """forward VALUE of the 1-/2-bit branches incl. the detach trick (:203-242); the caller supplies the identity gradient"""
    m = torch.mean(abs(w)) if layerwise else torch.mean(abs(w), dim=1, keepdim=True)
    if w_bits == 1:
        q = m * torch.sign(w / m)
    else:
        sc, nb, cv = 2 * m, 2 ** (w_bits - 1), 1 - 1e-2
        q = sc * (torch.round(torch.clamp(w / sc, -cv, cv) * nb - 0.5) + 0.5) / nb
    return q - w + w


def rms_norm(x, w, eps):
    """LlamaRMSNorm.forward (models/modeling_llama_quant.py:121-129), differentiated by autograd as the reference's is"""
    variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(variance + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        x = x.to(w.dtype)
    return w * x


def swiglu(gate, up):
    """the middle of LlamaMLP.forward (models/modeling_llama_quant.py:235) with act_fn = SiLU, differentiated by autograd as the reference's is"""
    return torch.nn.functional.silu(gate) * up


def rope(q, k, cos, sin, position_ids=None):
    """apply_rotary_pos_emb (models/modeling_llama_quant.py:181-196) with the cast of the tables to the tensors' dtype that the rotary module
    makes in front of it (:176-177; where q and k differ in dtype, one of them is float32 and so are the tables, as v's dtype makes them
    there), differentiated by autograd as the reference's is; position_ids None: the token index"""
    D = q.shape[-1]
    dt = q.dtype if q.dtype == k.dtype else torch.float32
    cos, sin = cos.reshape(-1, D).to(dtype=dt), sin.reshape(-1, D).to(dtype=dt)
    if position_ids is None:
        position_ids = torch.arange(q.shape[2], device=q.device).unsqueeze(0)
    cos, sin = cos[position_ids].unsqueeze(1), sin[position_ids].unsqueeze(1)

    def rotate_half(x):
        return torch.cat((-x[..., D // 2:], x[..., : D // 2]), dim=-1)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def attn_softmax(scores, mask, head_dim=None, scale=None):
    """the lines between the two attention products of LlamaAttention.forward (models/modeling_llama_quant.py:352-375), differentiated by
    autograd as the reference's are: the division by sqrt(head_dim) (a true division, as ATen's on the CPU; a given scale multiplies), the
    mask and the clamp where there is a mask, the fp32 softmax and its cast back"""
    attn = scores / math.sqrt(head_dim) if scale is None else scores * scale
    if mask is not None:
        attn = attn + mask
        attn = torch.max(attn, torch.tensor(torch.finfo(attn.dtype).min))
    return torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32).to(scores.dtype)


def _expand_kv(q, k, v):
    """grouped-query attention: k, v of Hkv heads with every head repeated H / Hkv times (query head h reads K/V head h // (H // Hkv))"""
    g = q.shape[1] // k.shape[1]
    return (k, v) if g == 1 else (k.repeat_interleave(g, 1), v.repeat_interleave(g, 1))


def attn_decode(q, k, v, mask, head_dim=None, scale=None):
    """both attention products of LlamaAttention.forward with the chain between them (models/modeling_llama_quant.py:345-377), in torch
    ops, under decode_attention's contract: the chain's roundings up to the clamp, then the fp32 softmax kept in fp32, the second product
    in float64 and ONE rounding to the dtype -> [B, H, T, D] as a view of [B, T, H, D] memory, as the device route returns it"""
    k, v = _expand_kv(q, k, v)
    attn = torch.matmul(q, k.transpose(2, 3))
    attn = attn / math.sqrt(head_dim) if scale is None else attn * scale
    if mask is not None:
        attn = attn + mask
        attn = torch.max(attn, torch.tensor(torch.finfo(attn.dtype).min))
    p = torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32)
    return torch.matmul(p.double(), v.double()).to(q.dtype).transpose(1, 2).contiguous().transpose(1, 2)


def attn_kv_decode(q, k_codes, k_t2, v_codes, v_t2, mask, inv, num_bits, rotary=None, key_positions=None):
    """kv_decode_attention in torch ops: the cache unpacked, divided by t2 in fp32, rounded to q's dtype and (k) rotated with the eager
    chain's roundings, then attn_decode's chain"""
    from . import ops
    k = ops.kv_codes_materialize(k_codes, k_t2, q.dtype, num_bits, rotary, key_positions)
    v = ops.kv_codes_materialize(v_codes, v_t2, q.dtype, num_bits)
    return attn_decode(q, k, v, mask, scale=inv)


def attn_prefill(q, k, v, mask, head_dim=None, scale=None, causal=False):
    """attn_decode for any T, under prefill_attention's contract; causal: the keys past S - T + t of row t get weight exactly 0 (-inf in
    front of the softmax) and the others go through the chain without a mask"""
    if not causal:
        return attn_decode(q, k, v, mask, head_dim, scale)
    T, S = q.shape[2], k.shape[2]
    k, v = _expand_kv(q, k, v)
    attn = torch.matmul(q, k.transpose(2, 3))
    attn = attn / math.sqrt(head_dim) if scale is None else attn * scale
    hidden = torch.arange(S)[None] > (S - T + torch.arange(T))[:, None]
    p = torch.nn.functional.softmax(attn.float().masked_fill(hidden, float("-inf")), dim=-1)
    return torch.matmul(p.double(), v.double()).to(q.dtype).transpose(1, 2).contiguous().transpose(1, 2)


def attn_cached(q, k_new, v_new, k_cache, v_cache, cache_lens, inv, cache_starts=None):
    """cached_decode_attention in torch ops that never read a length on the host: an index_put of the new rows at lens + arange(T) (into
    the caches extended by T rows, so that a row past Smax has somewhere to go: it takes part and is not kept), the seen / unseen mask
    from arange against lens and starts, and attn_prefill's causal chain over all Smax + T rows"""
    B, Hkv, T, D = k_new.shape
    Smax = k_cache.shape[2]
    lens = cache_lens.long().clamp(0, Smax)
    starts = torch.zeros_like(lens) if cache_starts is None else torch.minimum(cache_starts.long().clamp(min=0), lens)
    rows = lens[:, None] + torch.arange(T, device=q.device)      # [B, T]
    batch = torch.arange(B, device=q.device)[:, None]
    full = []
    for cache, new in ((k_cache, k_new), (v_cache, v_new)):
        ext = torch.cat([cache, cache.new_zeros((B, Hkv, T, D))], 2)
        ext[batch, :, rows] = new.transpose(1, 2)
        cache.copy_(ext[:, :, :Smax])
        full.append(ext)
    k, v = _expand_kv(q, *full)
    attn = torch.matmul(q, k.transpose(2, 3)) * inv
    col = torch.arange(Smax + T, device=q.device)
    hidden = (col < starts[:, None, None]) | (col > rows[:, :, None])      # [B, T, Smax + T]
    p = torch.nn.functional.softmax(attn.float().masked_fill(hidden[:, None], float("-inf")), dim=-1)
    return torch.matmul(p.double(), v.double()).to(q.dtype).transpose(1, 2).contiguous().transpose(1, 2)


def attn_cached_codes(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens, inv, num_bits,
                      rotary=None, cache_starts=None):
    """cached_kv_decode_attention in torch ops that never read a length on the host: attn_cached's index_put of the new code rows and
    divisors (into caches extended by T rows), the extended caches materialised as attn_kv_decode does with key s at position
    s - start, and attn_cached's seen / unseen mask and chain over all Smax + T rows"""
    from . import ops
    B, Hkv, T, _ = k_codes_new.shape
    Smax = k_code_cache.shape[2]
    lens = cache_lens.long().clamp(0, Smax)
    starts = torch.zeros_like(lens) if cache_starts is None else torch.minimum(cache_starts.long().clamp(min=0), lens)
    rows = lens[:, None] + torch.arange(T, device=q.device)      # [B, T]
    batch = torch.arange(B, device=q.device)[:, None]
    col = torch.arange(Smax + T, device=q.device)
    full = []
    for codes, t2, codes_new, t2_new in ((k_code_cache, k_t2_cache, k_codes_new, k_t2_new), (v_code_cache, v_t2_cache, v_codes_new, v_t2_new)):
        ext = torch.cat([codes, codes.new_zeros((B, Hkv, T, codes.shape[3]))], 2)
        ext[batch, :, rows] = codes_new.transpose(1, 2)
        codes.copy_(ext[:, :, :Smax])
        ext_t2 = torch.cat([t2, t2.new_ones((B, T))], 1)
        ext_t2[batch, rows] = t2_new
        t2.copy_(ext_t2[:, :Smax])
        if rotary is not None and codes is k_code_cache:
            pos = (col[None] - starts[:, None]).clamp(0, rotary[0].shape[-2] - 1)
            full.append(ops.kv_codes_materialize(ext, ext_t2, q.dtype, num_bits, rotary, pos))
        else:
            full.append(ops.kv_codes_materialize(ext, ext_t2, q.dtype, num_bits))
    k, v = _expand_kv(q, *full)
    attn = torch.matmul(q, k.transpose(2, 3)) * inv
    hidden = (col < starts[:, None, None]) | (col > rows[:, :, None])      # [B, T, Smax + T]
    p = torch.nn.functional.softmax(attn.float().masked_fill(hidden[:, None], float("-inf")), dim=-1)
    return torch.matmul(p.double(), v.double().masked_fill(hidden.all(1)[:, None, :, None], 0.0)).to(q.dtype).transpose(1, 2).contiguous().transpose(1, 2)


def _ste(x, dtype):
    """x rounded to `dtype`, in x's own (float64) dtype, with the gradient of the identity"""
    return x + (x.to(dtype).to(x.dtype) - x).detach()


def attn_train(q, k, v, mask, inv, causal=False):
    """attn_prefill with a gradient, under train_attention's contract, differentiated by torch's autograd: the chain in float64 with
    its roundings in front of the softmax applied straight through (the values are the rounded chain's, the derivative the unrounded
    formula's), torch.max's own rule at the clamp, ONE rounding of the output and one of each gradient"""
    T, S = q.shape[2], k.shape[2]
    z = _ste(_ste(_ste(torch.matmul(q.double(), k.double().transpose(2, 3)), q.dtype) * inv, torch.float32), q.dtype)      # inv: the fp32 factor
    if mask is not None:
        P = torch.promote_types(q.dtype, mask.dtype)
        z = torch.max(_ste(z + mask.double(), P), torch.tensor(torch.finfo(P).min, dtype=torch.float64))
    if causal:
        z = z.masked_fill(torch.arange(S)[None] > (S - T + torch.arange(T))[:, None], float("-inf"))
    out = torch.matmul(torch.softmax(z, -1), v.double()).to(q.dtype)
    return out.transpose(1, 2).contiguous().transpose(1, 2)
