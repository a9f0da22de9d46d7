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
"""
import torch

from . import compiled, cpu_tensors, ops

__all__ = ["attn_softmax", "install", "convert"]


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


def _forward(self, lookup, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False):
    """LlamaAttention.forward through the parent's attribute names, with attn_softmax between the two products.  lookup(): the rotary
    function, found at call time where the parent's forward finds it."""
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


def _fused_class(parent, names):
    """a subclass of `parent` whose forward is _forward; names: the mapping in which apply_rotary_pos_emb is looked up at call time"""
    class LlamaAttention(parent):
        fused_attn_softmax = True

        def forward(self, hidden_states, attention_mask=None, position_ids=None, past_key_value=None, output_attentions=False, use_cache=False):
            return _forward(self, lambda: names["apply_rotary_pos_emb"], hidden_states, attention_mask, position_ids, past_key_value,
                            output_attentions, use_cache)

    LlamaAttention.__qualname__ = LlamaAttention.__name__ = getattr(parent, "__name__", "LlamaAttention")
    LlamaAttention.__module__ = getattr(parent, "__module__", LlamaAttention.__module__)
    return LlamaAttention


def install(namespace):
    """Replace the attribute LlamaAttention of a module object (the reference's models.modeling_llama_quant, whose decoder layers look
    the class up when they are built) with a subclass of it: the constructor, the parameters and the state_dict are the parent's; the
    forward runs the projections, the K / V hooks and the rotary call through the parent's names (apply_rotary_pos_emb is looked up in
    `namespace` at call time, so rope.install composes in either order), then the product, attn_softmax, the product and o_proj.
    past_key_value, use_cache and output_attentions are honoured (output_attentions returns the probabilities in the scores' dtype).
    -> the previous attribute: assign it back to undo.  Models built before the call keep their attention: convert() re-classes those."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    previous = namespace.LlamaAttention
    namespace.LlamaAttention = _fused_class(previous, vars(namespace))
    return previous


_NEEDS = ("q_proj", "k_proj", "v_proj", "o_proj", "rotary_emb", "num_heads", "head_dim")
_converted = {}      # parent class -> its fused subclass: one per class, so that type(m) is shared by a model's layers


def _is_attention(m):
    return not getattr(m, "fused_attn_softmax", False) and all(hasattr(m, n) for n in _NEEDS) and "apply_rotary_pos_emb" in getattr(type(m).forward, "__globals__", {})


def convert(model):
    """Re-class, in place, every module of `model` (itself included) that has q_proj, k_proj, v_proj, o_proj, rotary_emb, num_heads and
    head_dim, whose forward finds apply_rotary_pos_emb in its module, and that is not converted already: its class becomes the fused
    subclass of its class, the object, its parameters and its state_dict keys stay.  -> the number re-classed."""
    if not isinstance(model, torch.nn.Module):
        raise TypeError(f"convert: expected a torch.nn.Module, got {type(model).__name__}")
    n = 0
    for m in model.modules():
        if _is_attention(m):
            parent = type(m)
            if parent not in _converted:
                _converted[parent] = _fused_class(parent, parent.forward.__globals__)
            m.__class__ = _converted[parent]
            n += 1
    return n
