"""The rotary position embedding of q and k (the reference's apply_rotary_pos_emb, models/modeling_llama_quant.py:181-196, called at
:338-341), fused:

    cos = cos[position_ids].unsqueeze(1); sin = sin[position_ids].unsqueeze(1)
    q_embed = (q * cos) + (rotate_half(q) * sin);  k_embed = (k * cos) + (rotate_half(k) * sin)

The two gathers, the casts of the tables and the five elementwise ops per tensor become one forward HIP kernel for q and k together and
one backward HIP kernel that give the eager chain's bits.  The transposed Jacobian of a rotation is the rotation by the opposite angle,
so the backward needs the tables and the positions alone: neither q, k nor rotate_half of them is kept.

    from llm_qat_amd import rope
    previous = rope.install(models.modeling_llama_quant)    # no edit: LlamaAttention.forward looks the function up at call time
    models.modeling_llama_quant.apply_rotary_pos_emb = previous   # undo
"""
import torch

from . import _rope_node, compiled, cpu_tensors, ops

__all__ = ["apply_rotary_pos_emb", "rotary", "install"]


class _Rotary(torch.autograd.Function):
    """the node in Python: serves where the C++ node (_rope_node.py) is not built or switched off, and states what that one does"""

    @staticmethod
    def forward(ctx, q, k, cos, sin, position_ids, geom, need):
        qo, ko, cos, sin, pos, q, k = ops.rope_launch_forward(q, k, cos, sin, position_ids, geom)
        if need:                                         # no gradient can be asked for: nothing saved.  Neither q nor k ever is
            ctx.save_for_backward(*((cos, sin) if pos is None else (cos, sin, pos)))
            ctx.like = ((tuple(q.shape), tuple(q.stride()), q.dtype), (tuple(k.shape), tuple(k.stride()), k.dtype))
        return qo, ko

    @staticmethod
    def backward(ctx, dq_out, dk_out):
        need_dq, need_dk = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_dq or need_dk):
            return (None,) * 7
        cos, sin, *pos = ctx.saved_tensors
        dq, dk = ops.rope_backward(dq_out, dk_out, cos, sin, pos[0] if pos else None, ctx.like[0], ctx.like[1], need_dq, need_dk)   # a frozen side: no launch work
        return dq, dk, None, None, None, None, None


def rotary(q, k, cos, sin, position_ids=None):
    """-> (q_embed, k_embed) as the eager chain computes them, forward and backward, bit for bit: fp32 arithmetic in the chain's op order
    with the chain's roundings (each product and each sum is rounded to the dtype as the chain stores it).

    q [B, Hq, T, D] and k [B, Hk, T, D]: one dtype (float32, bfloat16 or float16) -- or, as under autocast behind the reference's fp32 K
    quantizer, one of them float32 beside float32 tables: the results are then float32 and the gradients have their tensor's dtype, as
    the chain's promotion makes them -- and one device, D even; a tensor whose last stride is 1 (the
    reference's transposed view over [B, T, H * D], a part of a fused qkv projection) is read where it lies, any other layout is copied
    once.  cos, sin: [P, D] or [1, 1, P, D] in that dtype or in float32 (then rounded to it in the kernel, as the reference's .to(dtype)
    does).  position_ids: int64 [B, T] or [1, T], None: the token index; negative positions count from the table's end, a position outside
    [-P, P) gives NaN in every head of that token.  The results are dense in their input's dimension order: the chain's own layout.  Only
    the tables and positions are saved, and nothing under no_grad; a side that does not require grad gets no gradient computed.  CPU
    tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the chain runs in torch ops."""
    geom = ops.check_rope(q, k, cos, sin, position_ids, "rotary")
    if q.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(q, "rotary")
        return cpu_tensors.rope(q, k, cos, sin, position_ids)
    if torch.compiler.is_compiling():
        return compiled.rope(q, k, cos, sin, position_ids)
    need = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad)
    node = _rope_node.load()
    if node is not None and q.device.type == "cuda":     # the C++ node: the same launches without Python in front of them
        D = geom[4]
        pos = ops._rope_positions(position_ids, geom[0])[0]
        return tuple(node.rotary(q, k, ops._rope_table(cos, D), ops._rope_table(sin, D), pos, need))
    return _Rotary.apply(q, k, cos, sin, position_ids, geom, need)


def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
    """the reference's function (models/modeling_llama_quant.py:188-196), its signature and its return value, through the fused kernels"""
    return rotary(q, k, cos, sin, position_ids)


def install(namespace):
    """Replace the attribute apply_rotary_pos_emb of a module object (the reference's models.modeling_llama_quant, whose
    LlamaAttention.forward looks the function up when it is called, so models that are already built are served too) with the fused one.
    -> the previous attribute: assign it back to undo."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    previous = namespace.apply_rotary_pos_emb
    namespace.apply_rotary_pos_emb = apply_rotary_pos_emb
    return previous
