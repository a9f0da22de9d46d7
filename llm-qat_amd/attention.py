"""The chain between the two attention products of a LLaMA decoder layer (the reference's LlamaAttention.forward,
models/modeling_llama_quant.py:352-375), fused:

    attn = torch.matmul(q, k.transpose(2, 3)) / math.sqrt(head_dim)
    attn = attn + attention_mask
    attn = torch.max(attn, torch.tensor(torch.finfo(attn.dtype).min))
    attn = softmax(attn, dim=-1, dtype=torch.float32).to(q.dtype)

Everything behind the product becomes one forward HIP kernel and one backward HIP kernel: no fp32 [B, H, T, S] tensor, and nothing saved
but the scores, the mask and two floats per row.

    from llm_qat_amd.attention import attn_softmax, convert, install
    previous = install(models.modeling_llama_quant)    # no edit: models built from now on use the fused forward
    convert(teacher)                                   # an existing model, in place

decode_attention fuses the two products as well where a few new tokens (T <= 16) attend to a long cache and no gradient is asked for
(DESIGN.md section 30): one stream over k and v.  install(..., decode=True) / convert(..., decode=True) route such calls to it.
cached_decode_attention is decode_attention over a preallocated cache that one launch appends to in place and attends over, with the
sequence lengths on the device; static_kv_cache makes such a cache from a prompt call's (k, v).
kv_decode_attention is decode_attention over a cache held as the exported integer codes of the fake-quantized k and v, dequantized and
rotated in registers; install(..., decode=True, kv_codes=True) makes use_cache=True return such a cache.
cached_kv_decode_attention is both at once: a preallocated cache of codes and divisors, appended to in place by the launch that attends
over it; static_kv_codes_cache makes such a cache from a prompt call's codes.
prefill_attention is the same operation for any T, a whole sequence or a long chunk over a cache: the teacher's
forward, an evaluation run, the prompt pass of generation.  install(..., prefill=True) / convert(..., prefill=True) route to it.
train_attention is prefill_attention with a gradient in q, k and v: the student's call.  Its backward recomputes the
scores tile by tile from two floats per row, so no [B, H, T, S] tensor exists in either direction.  install(..., train=True) /
convert(..., train=True) route the calls that need a gradient to it.
"""
import torch

from . import compiled, cpu_tensors, ops

__all__ = ["attn_softmax", "install", "convert"]      # the recorded star-import set; decode_attention, cached_decode_attention, static_kv_cache, kv_decode_attention, cached_kv_decode_attention, static_kv_codes_cache, prefill_attention and train_attention are public by name


class _AttnSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, mask, geom, need):
        y, stats, sc, mk = ops.attn_launch_forward(scores.detach(), mask, geom, need_stats=need)      # no gradient can be asked for: no stats
        if need:
            ctx.save_for_backward(sc, stats, *(() if mk is None else (mk,)))
            ctx.inv = geom[4]
        return y

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        scores, stats, *mask = ctx.saved_tensors
        return ops.attn_softmax_backward(g, scores, mask[0] if mask else None, stats, scale=ctx.inv), None, None, None


def attn_softmax(scores, attention_mask=None, head_dim=None, *, scale=None):
    """softmax(max(scores / sqrt(head_dim) + attention_mask, finfo.min), -1, float32) in the scores' dtype, as the reference's lines
    compute it on the device: fp32 arithmetic with the chain's roundings in front of the softmax (the product with the fp32 reciprocal
    of sqrt(head_dim) rounded to the dtype, the sum with the mask in the promoted dtype, the clamp at that dtype's finfo.min), then an fp32
    softmax rounded once.  Without a mask there is no clamp, as in the reference.  The softmax sums in another order than ATen's, so
    the result is held to an error bound against float64 beside the eager chain's own, not to its bits.  The gradient is
    the chain's autograd: its casts, and torch.max's rule (a tie, which is every element of a fully masked row, gets half).

    scores: [B, H, T, S], float32, bfloat16 or float16, on a CUDA device; attention_mask: None, or [B, 1, T, S] / [1, 1, T, S] in the
    scores' dtype or float32 (the chain then promotes), read where it lies with a last stride of 1; it must not require grad.  Give
    head_dim, or scale= (the factor itself).  A non-contiguous scores tensor is copied once.  Only the scores, the mask and an fp32
    [rows, 2] are saved, and nothing under no_grad.  A NaN or +inf stays in its row.  CPU tensors are refused unless
    llm_qat_amd.allow_cpu_tensors(True): then the chain runs in torch ops."""
    geom = ops.check_attn_softmax(scores, attention_mask, head_dim, scale, "attn_softmax")
    if attention_mask is not None and attention_mask.requires_grad:
        raise ValueError("attn_softmax: a mask that requires grad is not served (the kernels compute no gradient for it)")
    if scores.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(scores, "attn_softmax")
        return cpu_tensors.attn_softmax(scores, attention_mask, head_dim, scale)
    if torch.compiler.is_compiling():
        return compiled.attn_softmax(scores, attention_mask, geom[4])
    need = torch.is_grad_enabled() and scores.requires_grad
    return _AttnSoftmax.apply(scores, attention_mask, geom, need)


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def decode_attention(q, k, v, attention_mask=None, head_dim=None, *, scale=None):
    """softmax(max(q k^T / sqrt(head_dim) + attention_mask, finfo.min), -1, float32) v for a few query rows over many keys, fused: the
    scores never exist in memory, k and v are read once.  The chain's roundings stand in front of the softmax as in attn_softmax (the
    first product rounded to the dtype, the product with the fp32 reciprocal of sqrt(head_dim), the sum with the mask in the promoted
    dtype, the clamp under a mask only); the softmax is online in fp32 and the unnormalised exponentials are the second product's
    operand, so the result is held to an error bound against float64 beside the composed path's own, not to its bits.

    q: [B, H, T, D] with T <= 16 and D of 64 or 128; k, v: [B, H, S, D]; all three bfloat16 or all three float16, on a CUDA device, read
    where they lie (the transposed views of a projection, a concatenation with a cache); attention_mask: None, or [B, 1, T, S] /
    [1, 1, T, S] in their dtype or float32.  Grouped-query attention: k, v may be [B, Hkv, S, D] with Hkv dividing H; query head h then
    attends to K/V head h // (H // Hkv), the repeat_interleave(k, H // Hkv, dim=1) convention, and the query heads of a group share one
    workgroup, so k and v are still read once.  Give head_dim, or scale=.  -> [B, H, T, D] as a view of [B, T, H, D] memory, so that
    .transpose(1, 2).reshape(B, T, H * D) is a view.  Forward only: a call in which a gradient is required raises.  CPU tensors are
    refused unless llm_qat_amd.allow_cpu_tensors(True): then the chain runs in torch ops."""
    B, H, T, S, D, inv = ops.check_attn_decode(q, k, v, attention_mask, head_dim, scale, "decode_attention")
    if _needs_grad(q, k, v, attention_mask):
        raise RuntimeError("decode_attention: forward only, but an input requires grad: call it under torch.no_grad(), detach the inputs, "
                           "or use the products around attn_softmax, which have a backward")
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "decode_attention")
        return cpu_tensors.attn_decode(q, k, v, attention_mask, head_dim, scale)
    if torch.compiler.is_compiling():
        return compiled.attn_decode(q, k, v, attention_mask, inv).transpose(1, 2)
    return ops.attn_decode_forward(q, k, v, attention_mask, scale=inv).transpose(1, 2)


def cached_decode_attention(q, k_new, v_new, k_cache, v_cache, cache_lens, head_dim=None, *, scale=None, cache_starts=None):
    """decode_attention over a preallocated K/V cache that is appended to IN PLACE, with the sequence lengths on the device (DESIGN.md
    section 35).  For batch row b with len = cache_lens[b], one launch (1) writes k_new[b], v_new[b] into rows len .. len + T - 1 of
    k_cache[b], v_cache[b], bit for bit, and (2) lets query row t attend to the keys cache_starts[b] <= s <= len + t of the updated cache:
    every earlier valid key, causal among the new tokens.  The result is what prefill_attention(q[b], cat(cache[b, :, :len], new[b]), ...,
    causal=True) defines: the no-mask chain (both roundings in front of the softmax, no clamp), unseen keys -inf behind it, the online
    fp32 softmax, the rounded exponentials as the second product's operand, one output rounding.  No torch.cat, no mask tensor, and the
    lengths are never read on the host: the grid and the workspace depend on the shapes alone, so a decode loop launches the same thing
    every step, and a batch may hold sequences of different lengths.

    q: [B, H, T, D], T <= 16, D of 64 or 128; k_new, v_new: [B, Hkv, T, D], Hkv dividing H, k already rotated, read where they lie (the
    transposed views of a projection); k_cache, v_cache: [B, Hkv, Smax, D] with a last stride of 1 and any other strides, never copied; all
    five bfloat16 or all five float16 on one CUDA device, the new tensors not overlapping the caches; cache_lens: int32 [B] on that device;
    cache_starts: None or int32 [B], keys below it are not seen (left padding).  The contract is 0 <= start <= len and len + T <= Smax; the
    kernel cannot tell the host, so it clamps: a negative length counts as 0, one above Smax as Smax, and a new row that would land at or
    past Smax is not stored but still attended to in this call.  cache_lens is NOT advanced: the caller adds T once, after its layers.
    Give head_dim, or scale=.  -> [B, H, T, D] as a view of [B, T, H, D] memory.  Forward only: a call in which a gradient is required
    raises.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then torch ops run, without a host read either."""
    geom = ops.check_attn_cached(q, k_new, v_new, k_cache, v_cache, cache_lens, head_dim, scale, cache_starts, "cached_decode_attention")
    if _needs_grad(q, k_new, v_new, k_cache, v_cache):
        raise RuntimeError("cached_decode_attention: forward only, but an input requires grad: call it under torch.no_grad(), detach the inputs, "
                           "or use the products around attn_softmax, which have a backward")
    inv = geom[6]
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "cached_decode_attention")
        return cpu_tensors.attn_cached(q, k_new, v_new, k_cache, v_cache, cache_lens, inv, cache_starts)
    if torch.compiler.is_compiling():
        return compiled.attn_cached(q, k_new, v_new, k_cache, v_cache, cache_lens, cache_starts, inv).transpose(1, 2)
    return ops.attn_cached_forward(q, k_new, v_new, k_cache, v_cache, cache_lens, scale=inv, cache_starts=cache_starts).transpose(1, 2)


def static_kv_cache(k, v, max_len):
    """(k, v) [B, Hkv, S, D] as a prompt call returned them -> (k_cache, v_cache, cache_lens) for cached_decode_attention: contiguous
    [B, Hkv, max_len, D] caches holding the prompt's rows in front (the rest zero) and int32 lengths [B], all S, on k's device."""
    if not isinstance(max_len, int) or isinstance(max_len, bool):
        raise TypeError(f"static_kv_cache: max_len is an int, got {type(max_len).__name__}")
    if k.dim() != 4 or k.shape != v.shape or k.dtype != v.dtype or k.device != v.device:
        raise ValueError(f"static_kv_cache: k and v are one [B, Hkv, S, D] of one dtype on one device, got {tuple(k.shape)} and {tuple(v.shape)}")
    B, Hkv, S, D = k.shape
    if max_len < S:
        raise ValueError(f"static_kv_cache: max_len={max_len} is below the prompt's S={S}")
    caches = []
    for t in (k, v):
        cache = t.new_zeros((B, Hkv, max_len, D))
        cache[:, :, :S] = t.detach()
        caches.append(cache)
    return caches[0], caches[1], torch.full((B,), S, dtype=torch.int32, device=k.device)


def kv_decode_attention(q, k_codes, k_t2, v_codes, v_t2, attention_mask=None, head_dim=None, *, scale=None, num_bits=8, rotary=None, key_positions=None):
    """decode_attention(q, k, v, ...) over a K/V cache held as the integer codes ops.sym_export writes for the per-token K / V hooks
    (DESIGN.md section 33): k = rope(rb(k_codes / k_t2)) and v = rb(v_codes / v_t2) are made in registers and never exist in memory, so
    the stream over the cache is a half (int8) or a quarter (int4) of the 16-bit one.  The dequantized values are QuantExport.dequantize()'s
    bits, the rotated key has the bits rope.rotary would have written, and everything behind the operands is decode_attention's.

    q: [B, H, T, D], bfloat16 or float16, T <= 16, D of 64 or 128; k_codes, v_codes: [B, H, S, D] int8, or for num_bits <= 4 uint8
    [B, H, S, D / 2] with element 2 k in the low nibble of byte k, read where they lie (the .view(b, s, nh, hd).transpose(1, 2) of an
    export's bins, a concatenation along the key axis); k_t2, v_t2: float32 [B, S], column 1 of QuantExport.scales; rotary: None (the codes
    are the final key's) or (cos, sin) tables [P, D] / [1, 1, P, D] in q's dtype or float32; key_positions: int64 [B, S] or [1, S], None:
    key s at position s (then S <= P).  v is never rotated.  Grouped-query attention: the codes may have Hkv heads, Hkv dividing H, as
    decode_attention's k, v; the heads of a group share one dequantisation and rotation of K (the divisors, tables and positions are per
    token).  -> [B, H, T, D] as a view of [B, T, H, D] memory.  Forward only: a call in
    which a gradient is required raises.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then torch ops run."""
    geom = ops.check_attn_kvdecode(q, k_codes, k_t2, v_codes, v_t2, attention_mask, head_dim, scale, num_bits, rotary, key_positions, "kv_decode_attention")
    if _needs_grad(q, k_t2, v_t2, attention_mask, *(rotary or ())):
        raise RuntimeError("kv_decode_attention: forward only, but an input requires grad: call it under torch.no_grad(), detach the inputs, "
                           "or use the products around attn_softmax, which have a backward")
    inv = geom[5]
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "kv_decode_attention")
        return cpu_tensors.attn_kv_decode(q, k_codes, k_t2, v_codes, v_t2, attention_mask, inv, num_bits, rotary, key_positions)
    if torch.compiler.is_compiling():
        cos, sin = rotary if rotary is not None else (None, None)
        return compiled.attn_kv_decode(q, k_codes, k_t2, v_codes, v_t2, attention_mask, inv, num_bits, cos, sin, key_positions).transpose(1, 2)
    return ops.attn_kvdecode_forward(q, k_codes, k_t2, v_codes, v_t2, attention_mask, scale=inv, num_bits=num_bits, rotary=rotary,
                                     key_positions=key_positions).transpose(1, 2)


def cached_kv_decode_attention(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens,
                               head_dim=None, *, scale=None, num_bits=8, rotary=None, cache_starts=None):
    """cached_decode_attention over a cache held as kv_decode_attention's integer codes: the preallocated caches are
    the codes and one float32 divisor per token, appended to IN PLACE, with the sequence lengths on the device.  For batch row b with
    len = cache_lens[b], one launch (1) writes the new code rows and the new divisors, bit for bit, into rows len .. len + T - 1 of the
    four caches and (2) lets query row t attend to the keys cache_starts[b] <= s <= len + t of the updated cache.  The operands are
    kv_decode_attention's, k = rope(rb(code / t2)) and v = rb(code / t2), made in registers; everything behind them is
    cached_decode_attention's: no mask, no clamp, unseen keys -inf behind the score, the online fp32 softmax.  No torch.cat, no mask tensor,
    no host read: a decode loop launches the same thing every step.

    q: [B, H, T, D], bfloat16 or float16, T <= 16, D of 64 or 128, read where it lies; k_codes_new, v_codes_new: [B, Hkv, T, D] int8, or for
    num_bits <= 4 uint8 [B, Hkv, T, D / 2] in ops.sym_export's nibble order, Hkv dividing H, read where they lie (the
    .view(b, t, nh, -1).transpose(1, 2) of an export's bins); k_t2_new, v_t2_new: float32 [B, T]; k_code_cache, v_code_cache:
    [B, Hkv, Smax, D or D / 2] with a last stride of 1 and any other strides, never copied; k_t2_cache, v_t2_cache: float32 [B, Smax] with
    a last stride of 1; cache_lens, cache_starts: int32 [B] on the device, as in cached_decode_attention; rotary: None (the codes are the
    final key's) or (cos, sin) tables [P, D] / [1, 1, P, D] in q's dtype or float32 with P >= Smax.  Key s of batch row b sits at position
    s - cache_starts[b], which is what cumulative-sum position ids give under left padding.  There is no positions tensor: a cache of
    arbitrary positions is out of scope (kv_decode_attention's key_positions serves it, over a torch.cat cache).  The contract is
    0 <= start <= len and len + T <= Smax; the kernel clamps lengths and starts and never trusts them, and a new row that would land at or
    past Smax is not stored but still attended to in this call.  cache_lens is NOT advanced.  Give head_dim, or scale=.
    -> [B, H, T, D] as a view of [B, T, H, D] memory.  Forward only: a call in which a gradient is required raises.  CPU tensors are
    refused unless llm_qat_amd.allow_cpu_tensors(True): then torch ops run, without a host read either."""
    geom = ops.check_attn_cached_codes(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens,
                                       head_dim, scale, num_bits, rotary, cache_starts, "cached_kv_decode_attention")
    if _needs_grad(q, k_t2_new, v_t2_new, k_t2_cache, v_t2_cache, *(rotary or ())):
        raise RuntimeError("cached_kv_decode_attention: forward only, but an input requires grad: call it under torch.no_grad(), detach the inputs, "
                           "or use the products around attn_softmax, which have a backward")
    inv = geom[6]
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "cached_kv_decode_attention")
        return cpu_tensors.attn_cached_codes(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens,
                                             inv, num_bits, rotary, cache_starts)
    if torch.compiler.is_compiling():
        cos, sin = rotary if rotary is not None else (None, None)
        return compiled.attn_cached_codes(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens,
                                          cache_starts, inv, num_bits, cos, sin).transpose(1, 2)
    return ops.attn_cached_codes_forward(q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens,
                                         scale=inv, num_bits=num_bits, rotary=rotary, cache_starts=cache_starts).transpose(1, 2)


def static_kv_codes_cache(k_codes, k_t2, v_codes, v_t2, max_len):
    """The codes cache a prompt call with kv_codes=True returned, k_codes, v_codes [B, Hkv, S, D or D / 2] and k_t2, v_t2 [B, S] ->
    (k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens) for cached_kv_decode_attention: contiguous [B, Hkv, max_len, ..] code
    caches and [B, max_len] divisor caches holding the prompt's rows in front (the other codes 0, the other divisors 1) and int32
    lengths [B], all S, on the codes' device."""
    if not isinstance(max_len, int) or isinstance(max_len, bool):
        raise TypeError(f"static_kv_codes_cache: max_len is an int, got {type(max_len).__name__}")
    if k_codes.dim() != 4 or k_codes.shape != v_codes.shape or k_codes.dtype != v_codes.dtype or k_codes.device != v_codes.device:
        raise ValueError(f"static_kv_codes_cache: k_codes and v_codes are one [B, Hkv, S, D or D / 2] of one dtype on one device, got {tuple(k_codes.shape)} "
                         f"and {tuple(v_codes.shape)}")
    B, Hkv, S, W = k_codes.shape
    if tuple(k_t2.shape) != (B, S) or tuple(v_t2.shape) != (B, S):
        raise ValueError(f"static_kv_codes_cache: the divisors are [{B}, {S}], got {tuple(k_t2.shape)} and {tuple(v_t2.shape)}")
    if max_len < S:
        raise ValueError(f"static_kv_codes_cache: max_len={max_len} is below the prompt's S={S}")
    caches = []
    for codes, t2 in ((k_codes, k_t2), (v_codes, v_t2)):
        code_cache, t2_cache = codes.new_zeros((B, Hkv, max_len, W)), t2.new_ones((B, max_len))
        code_cache[:, :, :S], t2_cache[:, :S] = codes.detach(), t2.detach()
        caches += [code_cache, t2_cache]
    return (*caches, torch.full((B,), S, dtype=torch.int32, device=k_codes.device))


def prefill_attention(q, k, v, attention_mask=None, head_dim=None, *, scale=None, causal=False):
    """decode_attention's operation, arithmetic and contract for any number T of query rows, fused: a workgroup owns 128 query rows and
    walks all keys, each tile of k and v staged once for its four waves; the scores never exist in memory, where the three calls write and
    re-read a [B, H, T, S] tensor twice.

    q: [B, H, T, D] with D of 64 or 128; k, v: [B, H, S, D]; all three bfloat16 or all three float16, on a CUDA device, read where they
    lie; attention_mask: None, or [B, 1, T, S] / [1, 1, T, S] in their dtype or float32.  causal=True (no mask, T <= S): query row t
    attends to the keys s <= S - T + t and to no others, which for finite scores is the additive causal mask's result; no mask is read
    and the keys past a workgroup's last row are skipped.  Grouped-query attention: k, v may be [B, Hkv, S, D] with Hkv dividing H,
    query head h over K/V head h // (H // Hkv); the result has the bits of the call on the repeated k, v.  Give head_dim, or scale=.
    -> [B, H, T, D] as a view of [B, T, H, D] memory.  Forward only: a call in which a gradient is required raises.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True):
    then the chain runs in torch ops."""
    B, H, T, S, D, inv = ops.check_attn_prefill(q, k, v, attention_mask, head_dim, scale, causal, "prefill_attention")
    if _needs_grad(q, k, v, attention_mask):
        raise RuntimeError("prefill_attention: forward only, but an input requires grad: call it under torch.no_grad(), detach the inputs, "
                           "or use the products around attn_softmax, which have a backward")
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "prefill_attention")
        return cpu_tensors.attn_prefill(q, k, v, attention_mask, head_dim, scale, causal)
    if torch.compiler.is_compiling():
        return compiled.attn_prefill(q, k, v, attention_mask, inv, causal).transpose(1, 2)
    return ops.attn_prefill_forward(q, k, v, attention_mask, scale=inv, causal=causal).transpose(1, 2)


class _TrainAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, inv, causal):
        out, stats, (qs, ks, vs, mk) = ops.attn_train_forward(q, k, v, mask, scale=inv, causal=causal)
        ctx.save_for_backward(qs, ks, vs, out, stats, *(() if mk is None else (mk,)))      # q, k, v, out, stats and the mask: nothing else
        ctx.inv, ctx.causal = inv, causal
        return out.transpose(1, 2)

    @staticmethod
    def backward(ctx, g):
        q, k, v, out, stats, *mask = ctx.saved_tensors
        grads = ops.attn_train_backward(g, q, k, v, mask[0] if mask else None, out.transpose(1, 2), stats, scale=ctx.inv, causal=ctx.causal)
        return (*(d.transpose(1, 2) if need else None for d, need in zip(grads, ctx.needs_input_grad)), None, None, None)


def train_attention(q, k, v, attention_mask=None, head_dim=None, *, scale=None, causal=False):
    """prefill_attention's operation, arithmetic and contract, differentiable in q, k and v.  The forward is
    prefill_attention's kernel, to the bit, and also writes the maximum and the sum of every query row (an fp32 [B, H, T, 2]); the backward
    is two kernels that recompute the scores and the probabilities tile by tile from those, q, k, v and the mask, so the only tensors saved
    are q, k, v, the mask, out and that pair, and no [B, H, T, S] tensor exists.  The gradient is the chain's: straight through its
    roundings, torch.max's rule at the clamp (a tie, which is every key of a fully masked row, gets half), held to an error bound against
    float64 beside the composed path's own, not to its bits.  No atomics: two backward calls give the same bits.

    q: [B, H, T, D] with D of 64 or 128; k, v: [B, H, S, D]; all three bfloat16 or all three float16, on a CUDA device, read where they
    lie; attention_mask: None, or [B, 1, T, S] / [1, 1, T, S] in their dtype or float32, which must not require grad; causal=True (no
    mask, T <= S) as prefill_attention's.  Give head_dim, or scale=.  -> [B, H, T, D] as a view of [B, T, H, D] memory; the gradients are
    views of [B, T, H, D] / [B, S, H, D] memory likewise.  Under no_grad, or where nothing requires grad, nothing is saved and no row
    statistics are written.  k, v of fewer heads than q (grouped-query attention) are refused: the backward does not serve them; expand
    k and v with repeat_interleave for a gradient.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the chain
    runs in torch ops."""
    B, H, T, S, D, inv = ops.check_attn_train(q, k, v, attention_mask, head_dim, scale, causal, "train_attention")
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "train_attention")
        return cpu_tensors.attn_train(q, k, v, attention_mask, inv, causal)
    if torch.compiler.is_compiling():
        return compiled.attn_train(q, k, v, attention_mask, inv, causal).transpose(1, 2)
    if not _needs_grad(q, k, v):
        return ops.attn_train_forward(q, k, v, attention_mask, scale=inv, causal=causal, need_stats=False)[0].transpose(1, 2)
    return _TrainAttention.apply(q, k, v, attention_mask, inv, causal)


def _fused_serves(q, k, v, attention_mask, hd, output_attentions, grad=False):
    return (not output_attentions and hd in ops.DECODE_HEAD_DIMS and q.dtype in (torch.bfloat16, torch.float16)
            and k.dtype == q.dtype and v.dtype == q.dtype and q.device.type == "cuda" and k.device == q.device and v.device == q.device
            and (attention_mask is None or (attention_mask.dtype in (q.dtype, torch.float32) and attention_mask.device == q.device))
            and _needs_grad(q, k, v, attention_mask) == grad and not (grad and attention_mask is not None and attention_mask.requires_grad))


def _forward(self, lookup, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False,
             decode=False, prefill=False, train=False, kv_codes=False):
    """LlamaAttention.forward through the parent's attribute names, with attn_softmax between the two products.  lookup(): the rotary
    function, found at call time where the parent's forward finds it.  decode: calls that decode_attention serves go to it, the others
    are counted (ops.decode_counts["fallback"]) and take the three calls.  prefill: calls that the decode route has not taken and
    prefill_attention serves go to it; the others are counted in ops.prefill_counts["fallback"], and a call the prefill route serves is
    a fallback of neither dict.  train: a call that needs a gradient and that train_attention serves goes to it; any other call that needs
    one is counted in ops.train_counts["fallback"].  kv_codes (with kv_bits <= 8): the cache is (k_codes, v_codes, k_t2, v_t2,
    key_positions), see _codes_forward."""
    if kv_codes and getattr(self, "kv_bits", 32) <= ops.KV_CODE_MAX_BITS:
        return _codes_forward(self, lookup, hidden_states, attention_mask, position_ids, past_key_value, output_attentions, use_cache, prefill, train)
    b, t, _ = hidden_states.size()
    nh, hd = self.num_heads, self.head_dim
    q = self.q_proj(hidden_states).view(b, t, nh, hd).transpose(1, 2)
    k = self.k_proj(hidden_states)
    v = self.v_proj(hidden_states)
    if getattr(self, "kv_bits", 32) < 32:      # per token across all heads, before the head split and the rotation
        k = self.act_quantizer_k.apply(k, self.act_clip_val_k, self.kv_bits, False)
        v = self.act_quantizer_v.apply(v, self.act_clip_val_v, self.kv_bits, False)
    k = k.view(b, t, nh, hd).transpose(1, 2)
    v = v.view(b, t, nh, hd).transpose(1, 2)
    s = t if past_key_value is None else t + past_key_value[0].shape[-2]
    cos, sin = self.rotary_emb(v, seq_len=s)
    q, k = lookup()(q, k, cos, sin, position_ids)
    if past_key_value is not None:
        k = torch.cat([past_key_value[0], k], dim=2)
        v = torch.cat([past_key_value[1], v], dim=2)
    past_key_value = (k, v) if use_cache else None
    return _attend(self, q, k, v, attention_mask, past_key_value, output_attentions, decode, prefill, train)


def _attend(self, q, k, v, attention_mask, past_key_value, output_attentions, decode, prefill, train):
    """_forward behind the cache: the routes over q [B, H, T, D] and the full k, v -> (output, probabilities or None, past_key_value)"""
    b, nh, t, hd = q.shape
    s = k.shape[2]
    if decode or prefill:
        serves = _fused_serves(q, k, v, attention_mask, hd, output_attentions)
        fused = decode_attention if decode and serves and t <= ops.DECODE_MAX_T else prefill_attention if prefill and serves else None
        if fused is not None:
            if attention_mask is not None and attention_mask.size() != (b, 1, t, s):
                raise ValueError(f"Attention mask should be of size {(b, 1, t, s)}, but is {attention_mask.size()}")
            out = fused(q, k, v, attention_mask, hd)
            return self.o_proj(out.transpose(1, 2).reshape(b, t, nh * hd)), None, past_key_value
        ops.decode_counts["fallback"] += int(decode)
        ops.prefill_counts["fallback"] += int(prefill)
    if train and _needs_grad(q, k, v, attention_mask):
        if _fused_serves(q, k, v, attention_mask, hd, output_attentions, grad=True):
            if attention_mask is not None and attention_mask.size() != (b, 1, t, s):
                raise ValueError(f"Attention mask should be of size {(b, 1, t, s)}, but is {attention_mask.size()}")
            out = train_attention(q, k, v, attention_mask, hd)
            return self.o_proj(out.transpose(1, 2).reshape(b, t, nh * hd)), None, past_key_value
        ops.train_counts["fallback"] += 1
    scores = torch.matmul(q, k.transpose(2, 3))
    if scores.size() != (b, nh, t, s):
        raise ValueError(f"Attention weights should be of size {(b, nh, t, s)}, but is {scores.size()}")
    if attention_mask is not None and attention_mask.size() != (b, 1, t, s):
        raise ValueError(f"Attention mask should be of size {(b, 1, t, s)}, but is {attention_mask.size()}")
    y = attn_softmax(scores, attention_mask, hd)
    out = torch.matmul(y, v)
    if out.size() != (b, nh, t, hd):
        raise ValueError(f"`attn_output` should be of size {(b, nh, t, hd)}, but is {out.size()}")
    out = self.o_proj(out.transpose(1, 2).reshape(b, t, nh * hd))
    return out, (y if output_attentions else None), past_key_value


def _codes_forward(self, lookup, hidden_states, attention_mask, position_ids, past_key_value, output_attentions, use_cache, prefill, train):
    """_forward with the cache held as codes: past_key_value = (k_codes, v_codes, k_t2, v_t2, key_positions), the
    codes [B, H, S, D] (int4: D / 2) views of ops.sym_export's bins of the k / v projection outputs (k before the rotation), t2 fp32 [B, S],
    the positions int64 [B, S]; each grows by torch.cat along its key axis.  A call with such a cache that kv_decode_attention serves goes
    to it with the module's rotary tables; any other one with a cache materialises it in torch ops (ops.kvdecode_counts["fallback"]) and
    takes the decode=True routes.  The prompt call runs on the fake-quantized tensors as ever and only emits the cache."""
    b, t, _ = hidden_states.size()
    nh, hd, bits = self.num_heads, self.head_dim, self.kv_bits
    q = self.q_proj(hidden_states).view(b, t, nh, hd).transpose(1, 2)
    kx, vx = self.k_proj(hidden_states), self.v_proj(hidden_states)
    k = self.act_quantizer_k.apply(kx, self.act_clip_val_k, bits, False).view(b, t, nh, hd).transpose(1, 2)
    v = self.act_quantizer_v.apply(vx, self.act_clip_val_v, bits, False).view(b, t, nh, hd).transpose(1, 2)
    p = 0 if past_key_value is None else past_key_value[0].shape[-2]
    s = t + p
    cos, sin = self.rotary_emb(v, seq_len=s)
    pos = (torch.arange(p, s, device=q.device) if position_ids is None else position_ids).reshape(-1, t).expand(b, t)
    cache = None
    if use_cache or past_key_value is not None:
        container = ops.kv_container(bits)
        new = []
        for x in (kx, vx):
            e = ops.sym_export(x.detach(), bits, container=container)
            new += [e.bins.view(b, t, nh, -1).transpose(1, 2), e.scales[:, 1].reshape(b, t)]
        new = (new[0], new[2], new[1], new[3], pos)
        cache = new if past_key_value is None else tuple(torch.cat([old, x], dim=-2 if i < 2 else 1) for i, (old, x) in enumerate(zip(past_key_value, new)))
    if past_key_value is None:
        q, k = lookup()(q, k, cos, sin, position_ids)
        return _attend(self, q, k, v, attention_mask, cache if use_cache else None, output_attentions, True, prefill, train)
    serves = (_fused_serves(q, k, v, attention_mask, hd, output_attentions) and t <= ops.DECODE_MAX_T and cos.dtype == q.dtype
              and cos.shape[-2] >= s and cos.device == q.device)
    if serves:
        if attention_mask is not None and attention_mask.size() != (b, 1, t, s):
            raise ValueError(f"Attention mask should be of size {(b, 1, t, s)}, but is {attention_mask.size()}")
        q = lookup()(q, k, cos, sin, position_ids)[0]
        out = kv_decode_attention(q, cache[0], cache[2], cache[1], cache[3], attention_mask, hd, num_bits=bits, rotary=(cos, sin), key_positions=cache[4])
        return self.o_proj(out.transpose(1, 2).reshape(b, t, nh * hd)), None, cache if use_cache else None
    ops.kvdecode_counts["fallback"] += 1
    q, k = lookup()(q, k, cos, sin, position_ids)
    old = past_key_value
    k = torch.cat([ops.kv_codes_materialize(old[0], old[2], q.dtype, bits, (cos, sin), old[4]), k], dim=2)
    v = torch.cat([ops.kv_codes_materialize(old[1], old[3], q.dtype, bits), v], dim=2)
    return _attend(self, q, k, v, attention_mask, cache if use_cache else None, output_attentions, True, prefill, train)


def _fused_class(parent, names, decode=False, prefill=False, train=False, kv_codes=False):
    """a subclass of `parent` whose forward is _forward; names: the mapping in which apply_rotary_pos_emb is looked up at call time"""
    class LlamaAttention(parent):
        fused_attn_softmax = True
        fused_attn_decode = decode
        fused_attn_prefill = prefill
        fused_attn_train = train
        fused_attn_kv_codes = kv_codes

        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False):
            return _forward(self, lambda: names["apply_rotary_pos_emb"], hidden_states, attention_mask, position_ids, past_key_value,
                            output_attentions, use_cache, decode, prefill, train, kv_codes)

    LlamaAttention.__qualname__ = LlamaAttention.__name__ = getattr(parent, "__name__", "LlamaAttention")
    LlamaAttention.__module__ = getattr(parent, "__module__", LlamaAttention.__module__)
    return LlamaAttention


def _check_kv_codes(kv_codes, decode, what):
    if kv_codes and not decode:
        raise ValueError(f"{what}: kv_codes=True keeps the cache for kv_decode_attention, which is a decode route: give decode=True as well")


def install(namespace, decode=False, prefill=False, train=False, kv_codes=False):
    """Replace the attribute LlamaAttention of a module object (the reference's models.modeling_llama_quant, whose decoder layers look
    the class up when they are built) with a subclass of it: the constructor, the parameters and the state_dict are the parent's; the
    forward runs the projections, the K / V hooks and the rotary call through the parent's names (apply_rotary_pos_emb is looked up in
    `namespace` at call time, so rope.install composes in either order), then the product, attn_softmax, the product and o_proj.
    past_key_value, use_cache and output_attentions are honoured (output_attentions returns the probabilities in the scores' dtype).
    decode=True: a call with at most 16 new tokens, a head_dim of 64 or 128, q, k, v sharing bfloat16 or float16 on the device, no
    output_attentions and no gradient to ask for goes to decode_attention; any other is counted in ops.decode_counts["fallback"].
    prefill=True: a call that meets the same conditions but for the number of tokens, and that the decode route has not taken, goes to
    prefill_attention with the module's mask (causality is never assumed); any other is counted in ops.prefill_counts["fallback"].
    train=True: a call that needs a gradient and meets the other conditions goes to train_attention with the module's mask; any other call
    that needs a gradient is counted in ops.train_counts["fallback"] and takes the three calls.
    kv_codes=True (needs decode=True; a module whose kv_bits is above 8 ignores it): use_cache=True returns past_key_value = (k_codes,
    v_codes, k_t2, v_t2, key_positions), the integer codes of the fake-quantized k and v (k before the rotation) with one divisor per
    token, and a call over such a cache goes to kv_decode_attention; one it cannot serve is counted in ops.kvdecode_counts["fallback"].
    -> the previous attribute: assign it back to undo.  Models built before the call keep their attention: convert() re-classes those."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    _check_kv_codes(kv_codes, decode, "install")
    previous = namespace.LlamaAttention
    namespace.LlamaAttention = _fused_class(previous, vars(namespace), bool(decode), bool(prefill), bool(train), bool(kv_codes))
    return previous


_NEEDS = ("q_proj", "k_proj", "v_proj", "o_proj", "rotary_emb", "num_heads", "head_dim")
_converted = {}      # (parent class, decode, prefill, train, kv_codes) -> its fused subclass: one per class, so that type(m) is shared by a model's layers


def _is_attention(m):
    return not getattr(m, "fused_attn_softmax", False) and all(hasattr(m, n) for n in _NEEDS) and "apply_rotary_pos_emb" in getattr(type(m).forward, "__globals__", {})


def convert(model, decode=False, prefill=False, train=False, kv_codes=False):
    """Re-class, in place, every module of `model` (itself included) that has q_proj, k_proj, v_proj, o_proj, rotary_emb, num_heads and
    head_dim, whose forward finds apply_rotary_pos_emb in its module, and that is not converted already: its class becomes the fused
    subclass of its class, the object, its parameters and its state_dict keys stay.  decode, prefill, train, kv_codes: as install's.  -> the number re-classed."""
    if not isinstance(model, torch.nn.Module):
        raise TypeError(f"convert: expected a torch.nn.Module, got {type(model).__name__}")
    _check_kv_codes(kv_codes, decode, "convert")
    n = 0
    for m in model.modules():
        if _is_attention(m):
            parent = type(m)
            key = (parent, bool(decode), bool(prefill), bool(train), bool(kv_codes))
            if key not in _converted:
                _converted[key] = _fused_class(parent, parent.forward.__globals__, *key[1:])
            m.__class__ = _converted[key]
            n += 1
    return n
