"""torch.compile entry of the drop-in (reachable in LLM-QAT through HF's `--torch_compile`, utils/kd_trainer.py:281-286).

The eager path launches the kernels through ctypes from inside `torch.autograd.Function`s, which Dynamo cannot trace
(every quantizer call is a graph break).  Here the same launches are registered as `torch.library` custom ops: opaque
to Dynamo, with a fake-tensor shape rule and an autograd formula, so a compiled `QuantizeLinear` / attention block is
ONE graph.  `utils_quant` routes here while `torch.compiler.is_compiling()`; results are the eager path's, bit for bit
(same kernels).  Data flow of the compiled path is the reference's (the backward re-reads the saved input, :45 / :83):
what a compiled graph keeps alive is planned by the partitioner, so the STE-mask / sharing / pairing machinery of the
eager path is not replicated here.
"""
from typing import List, Optional, Tuple

import torch

from . import ops

_KINDS = {"sym": 0, "asym": 1}


# mode: 0 = arithmetic in the tensor's own dtype; 1 = autocast arithmetic, result rounded once to the tensor dtype
# (QuantizeLinear's operands); 2 = autocast arithmetic, fp32 result (what the reference returns under autocast)
@torch.library.custom_op("llmqat_amd::fake_quant", mutates_args=(), device_types="cuda")
def fake_quant_op(x: torch.Tensor, clip: torch.Tensor, kind: int, num_bits: int, layerwise: bool, mode: int) -> torch.Tensor:
    if mode:
        return ops.sym_forward_autocast(x, num_bits, layerwise, wide=mode == 2)[0]
    return ops.sym_quantize(x, num_bits, layerwise) if kind == 0 else ops.asym_quantize(x, num_bits, layerwise)


@fake_quant_op.register_fake
def _(x, clip, kind, num_bits, layerwise, mode):
    if x.dim() > 4:
        raise ValueError(f"fake-quant expects at most 4 dimensions, got {x.dim()}")  # utils_quant.py:70
    return torch.empty_like(x, dtype=torch.float32 if mode == 2 else x.dtype)


@torch.library.custom_op("llmqat_amd::fake_quant_bwd", mutates_args=(), device_types="cuda")
def fake_quant_bwd(grad_output: torch.Tensor, x: torch.Tensor, clip: torch.Tensor) -> torch.Tensor:
    lo, hi = clip.tolist()[:2] if clip.dim() else (clip.item(),) * 2
    g = grad_output if grad_output.dtype == x.dtype else grad_output.to(x.dtype)  # autocast: fp32 gradient of the fp32 result
    return ops.ste_backward(g, x, float(lo), float(hi))


@fake_quant_bwd.register_fake
def _(grad_output, x, clip):
    return torch.empty_like(grad_output, dtype=x.dtype)


def _setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])  # reference :45 / :104: (input, clip_val)


def _backward(ctx, grad_output):
    x, clip = ctx.saved_tensors
    return fake_quant_bwd(grad_output, x, clip), None, None, None, None, None


fake_quant_op.register_autograd(_backward, setup_context=_setup)


@torch.library.custom_op("llmqat_amd::low_bit_weight", mutates_args=(), device_types="cuda")
def low_bit_weight_op(w: torch.Tensor, scale: torch.Tensor, w_bits: int) -> torch.Tensor:
    return ops.low_bit_weight(w, scale, w_bits)


@low_bit_weight_op.register_fake
def _(w, scale, w_bits):
    return torch.empty_like(w, memory_format=torch.contiguous_format)


low_bit_weight_op.register_autograd(lambda ctx, g: (g, None, None))  # the detach trick: identity gradient (:240-242)


def fake_quant(kind, x, clip_val, num_bits, layerwise, narrow=False):
    """SymQuantizer / AsymQuantizer .apply while compiling."""
    mode = 0
    if kind == "sym" and ops.autocast_active(x):
        mode = 1 if (narrow and ops.autocast_narrow_ok(x)) else 2
    return fake_quant_op(x, clip_val, _KINDS[kind], int(num_bits), bool(layerwise), mode)


# ---- MX block-scaled fake quantization (DESIGN.md sections 13, 15, 16, 17).  One op per combination of options (the names a traced graph
# holds); behind them one fake implementation, one straight-through gradient and one dispatcher (mx_fake_quant) -------------------------
def _mx_quant_fake(x, fmt, rotate=False, scale_rule="floor", mask=False, axis=-1):
    """the quantizer ops' fake implementation: ops.mx_quantize_axis's checks on shapes alone -> y (, the numel / 8 bytes of the bitmap)"""
    if axis == -2:
        ops.check_mx_cols(tuple(x.shape), fmt)
    else:
        ops.check_mx(tuple(x.shape), fmt)
    ops.check_mx_scale_rule(scale_rule)
    if rotate:
        ops.check_mx_rotate(tuple(x.shape), "mx_quantize")
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    return (y, x.new_empty((x.numel() // 8,), dtype=torch.uint8)) if mask else y


def _mx_straight_through(op, rotate=None):
    """the gradient of a quantizer op without a bitmap: the incoming one itself, times R (one rotate launch) where the op rotates -- a
    constant, or None: its `rotate` input says; nothing saved"""
    def setup(ctx, inputs, output):
        ctx.rotate, ctx.rest = (inputs[2] if rotate is None else rotate), (None,) * (len(inputs) - 1)

    op.register_autograd(lambda ctx, g: (mx_block_rotate_op(g) if ctx.rotate else g,) + ctx.rest, setup_context=setup)


# The block-Hadamard rotation (ops.mx_rotate): R is symmetric and its own inverse, so the gradient is the same op on the gradient
@torch.library.custom_op("llmqat_amd::mx_block_rotate", mutates_args=(), device_types="cuda")
def mx_block_rotate_op(x: torch.Tensor) -> torch.Tensor:
    return ops.mx_rotate(x)


@mx_block_rotate_op.register_fake
def _(x):
    ops.check_mx_rotate(tuple(x.shape))
    return torch.empty_like(x, memory_format=torch.contiguous_format)


mx_block_rotate_op.register_autograd(lambda ctx, g: mx_block_rotate_op(g))


# ops.mx_quantize(x, fmt): the identity gradient
@torch.library.custom_op("llmqat_amd::mx_fake_quant", mutates_args=(), device_types="cuda")
def mx_fake_quant_op(x: torch.Tensor, fmt: str) -> torch.Tensor:
    return ops.mx_quantize(x, fmt)


# ... of x R in one launch (rotate=True): grad_x = grad_y R
@torch.library.custom_op("llmqat_amd::mx_fake_quant_rot", mutates_args=(), device_types="cuda")
def mx_fake_quant_rot_op(x: torch.Tensor, fmt: str) -> torch.Tensor:
    return ops.mx_quantize(x, fmt, rotate=True)


# ... under a non-default scale rule
@torch.library.custom_op("llmqat_amd::mx_fake_quant_rule", mutates_args=(), device_types="cuda")
def mx_fake_quant_rule_op(x: torch.Tensor, fmt: str, rotate: bool, scale_rule: str) -> torch.Tensor:
    return ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=scale_rule)


# ... along axis -2, the blocks running down the columns (ops.mx_quantize_axis)
@torch.library.custom_op("llmqat_amd::mx_fake_quant_cols", mutates_args=(), device_types="cuda")
def mx_fake_quant_cols_op(x: torch.Tensor, fmt: str, scale_rule: str) -> torch.Tensor:
    return ops.mx_quantize_axis(x, fmt, scale_rule=scale_rule, axis=-2)


# ... with return_mask=True: (y, bitmap); the bitmap is all the backward keeps, and the backward is one launch
@torch.library.custom_op("llmqat_amd::mx_fake_quant_clip", mutates_args=(), device_types="cuda")
def mx_fake_quant_clip_op(x: torch.Tensor, fmt: str, rotate: bool, scale_rule: str) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=scale_rule, return_mask=True)


mx_fake_quant_op.register_fake(_mx_quant_fake)
mx_fake_quant_rot_op.register_fake(lambda x, fmt: _mx_quant_fake(x, fmt, True))
mx_fake_quant_rule_op.register_fake(_mx_quant_fake)
mx_fake_quant_cols_op.register_fake(lambda x, fmt, scale_rule: _mx_quant_fake(x, fmt, False, scale_rule, False, -2))
mx_fake_quant_clip_op.register_fake(lambda x, fmt, rotate, scale_rule: _mx_quant_fake(x, fmt, rotate, scale_rule, True))
_mx_straight_through(mx_fake_quant_op, False)
_mx_straight_through(mx_fake_quant_rot_op, True)
_mx_straight_through(mx_fake_quant_rule_op)
_mx_straight_through(mx_fake_quant_cols_op, False)


# ops.mx_ste_backward: the gradient under the saturation bitmap (rotate: times R, same launch)
@torch.library.custom_op("llmqat_amd::mx_ste_backward", mutates_args=(), device_types="cuda")
def mx_ste_backward_op(g: torch.Tensor, mask: torch.Tensor, rotate: bool) -> torch.Tensor:
    return ops.mx_ste_backward(g, mask, rotate)


@mx_ste_backward_op.register_fake
def _(g, mask, rotate):
    ops.check_mx_ste(tuple(g.shape), tuple(mask.shape), mask.dtype, rotate)
    return torch.empty_like(g, memory_format=torch.contiguous_format)


def _mx_clip_setup(ctx, inputs, output):
    ctx.rotate = inputs[2]
    ctx.save_for_backward(output[1])


def _mx_clip_backward(ctx, grad_y, grad_mask):
    return mx_ste_backward_op(grad_y, ctx.saved_tensors[0], ctx.rotate), None, None, None


mx_fake_quant_clip_op.register_autograd(_mx_clip_backward, setup_context=_mx_clip_setup)


def mx_fake_quant(x, fmt, rotate, scale_rule, clip, axis=-1):
    """utils_quant's MX quantizer while compiling: the op that serves (rotate, scale_rule, clip, axis)."""
    if axis == -2:
        if rotate or clip:
            raise ValueError("mx_fake_quant: the column axis (axis=-2) serves neither the rotation nor the clip gradient yet")
        return mx_fake_quant_cols_op(x, fmt, scale_rule)
    if clip:
        return mx_fake_quant_clip_op(x, fmt, rotate, scale_rule)[0]
    if scale_rule != "floor":
        return mx_fake_quant_rule_op(x, fmt, rotate, scale_rule)
    return mx_fake_quant_rot_op(x, fmt) if rotate else mx_fake_quant_op(x, fmt)


# ---- ops.mx_export as ops: (elements, scales) of x in `fmt` (mxfp4 / mxfp8_*); of x R under rotate; under a scale rule ------------------
def _mx_export_fake(x, fmt, rotate=False, scale_rule="floor"):
    ops.check_mx(tuple(x.shape), fmt)
    ops.check_mx_scale_rule(scale_rule, "mx_export")
    if rotate:
        ops.check_mx_rotate(tuple(x.shape), "mx_export")
    if fmt not in ops.MX_GEMM_FORMATS:
        raise ValueError(f"{fmt!r}: FP6 formats have no export packing")
    lead, cols = tuple(x.shape[:-1]), x.shape[-1]
    return (x.new_empty(lead + (cols // 2 if fmt == "mxfp4" else cols,), dtype=torch.uint8),
            x.new_empty(lead + (cols // ops.MX_BLOCK,), dtype=torch.uint8))


@torch.library.custom_op("llmqat_amd::mx_export", mutates_args=(), device_types="cuda")
def mx_export_op(x: torch.Tensor, fmt: str) -> Tuple[torch.Tensor, torch.Tensor]:
    e = ops.mx_export(x, fmt)
    return e.elements, e.scales


@torch.library.custom_op("llmqat_amd::mx_export_rot", mutates_args=(), device_types="cuda")
def mx_export_rot_op(x: torch.Tensor, fmt: str) -> Tuple[torch.Tensor, torch.Tensor]:
    e = ops.mx_export(x, fmt, rotate=True)
    return e.elements, e.scales


@torch.library.custom_op("llmqat_amd::mx_export_rule", mutates_args=(), device_types="cuda")
def mx_export_rule_op(x: torch.Tensor, fmt: str, rotate: bool, scale_rule: str) -> Tuple[torch.Tensor, torch.Tensor]:
    e = ops.mx_export(x, fmt, rotate=rotate, scale_rule=scale_rule)
    return e.elements, e.scales


mx_export_op.register_fake(_mx_export_fake)
mx_export_rot_op.register_fake(lambda x, fmt: _mx_export_fake(x, fmt, True))
mx_export_rule_op.register_fake(_mx_export_fake)


def mx_export(x, fmt, rotate, scale_rule):
    """MXLinear's activation export while compiling: the op that serves (rotate, scale_rule) -> (elements, scales)."""
    if scale_rule != "floor":
        return mx_export_rule_op(x, fmt, rotate, scale_rule)
    return mx_export_rot_op(x, fmt) if rotate else mx_export_op(x, fmt)


# MX block-scaled GEMM (ops.mx_matmul) on the tensors of the two exports; inference only: no autograd formula is registered, so asking
# for a gradient through it raises
@torch.library.custom_op("llmqat_amd::mx_matmul", mutates_args=(), device_types="cuda")
def mx_matmul_op(a_elems: torch.Tensor, a_scales: torch.Tensor, a_fmt: str, w_elems: torch.Tensor, w_scales: torch.Tensor, w_fmt: str,
                 a_shape: List[int], out_dtype: torch.dtype) -> torch.Tensor:
    return ops.mx_matmul_tensors(a_elems, a_scales, a_fmt, w_elems, w_scales, w_fmt, tuple(a_shape), out_dtype)


@mx_matmul_op.register_fake
def _(a_elems, a_scales, a_fmt, w_elems, w_scales, w_fmt, a_shape, out_dtype):
    _, N, _ = ops.check_mx_matmul(tuple(a_shape), a_fmt, (w_scales.shape[0], w_scales.shape[1] * ops.MX_BLOCK), w_fmt, out_dtype)
    return a_elems.new_empty(tuple(a_shape[:-1]) + (N,), dtype=out_dtype)


# ops.mx_dequantize on the export's tensors: the weight of MXLinear's dequantized route; inference only, as mx_matmul
@torch.library.custom_op("llmqat_amd::mx_dequant", mutates_args=(), device_types="cuda")
def mx_dequant_op(elements: torch.Tensor, scales: torch.Tensor, fmt: str, shape: List[int], dtype: torch.dtype) -> torch.Tensor:
    return ops.mx_dequantize_tensors(elements, scales, fmt, tuple(shape), dtype)


@mx_dequant_op.register_fake
def _(elements, scales, fmt, shape, dtype):
    ops.check_mx_dequant(fmt, tuple(shape), dtype)
    return elements.new_empty(tuple(shape), dtype=dtype)


# ---- the distillation loss (ops.kd_kl_forward / ops.kd_kl_backward): (loss, row_stats) and the student's gradient ----
@torch.library.custom_op("llmqat_amd::kd_kl_fwd", mutates_args=(), device_types="cuda")
def kd_kl_fwd_op(student: torch.Tensor, teacher: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    loss, row_stats, _ = ops.kd_kl_forward(student, teacher)
    return loss.clone(), row_stats.clone()      # the two are views of one side buffer: an op's outputs own their storage


@kd_kl_fwd_op.register_fake
def _(student, teacher):
    rows, _, _ = ops.check_kd(student, teacher)
    return student.new_empty((), dtype=torch.float32), student.new_empty((rows, 2), dtype=torch.float32)


@torch.library.custom_op("llmqat_amd::kd_kl_bwd", mutates_args=(), device_types="cuda")
def kd_kl_bwd_op(student: torch.Tensor, teacher: torch.Tensor, row_stats: torch.Tensor, grad_loss: torch.Tensor) -> torch.Tensor:
    return ops.kd_kl_backward(student, teacher, row_stats, grad_loss)


@kd_kl_bwd_op.register_fake
def _(student, teacher, row_stats, grad_loss):
    ops.check_kd(student, teacher)
    return torch.empty_like(student, memory_format=torch.contiguous_format)


def _kd_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1])


def _kd_backward(ctx, grad_loss, grad_stats):
    student, teacher, row_stats = ctx.saved_tensors
    return kd_kl_bwd_op(student, teacher, row_stats, grad_loss), None


kd_kl_fwd_op.register_autograd(_kd_backward, setup_context=_kd_setup)


def kd_kl_loss(student, teacher):
    """distill.kd_kl_loss while compiling"""
    return kd_kl_fwd_op(student, teacher)[0]


# ---- the language-model loss (ops.ce_forward / ops.ce_backward): (loss, row_lse, n_valid) and the logits' gradient ----
@torch.library.custom_op("llmqat_amd::ce_fwd", mutates_args=(), device_types="cuda")
def ce_fwd_op(logits: torch.Tensor, labels: torch.Tensor, shift: bool, ignore_index: int, reduction: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    loss, row_lse, _, n_valid = ops.ce_forward(logits, labels, shift, ignore_index, reduction)
    return loss.clone(), row_lse.clone(), n_valid.clone()      # the three are views of one side buffer: an op's outputs own their storage


@ce_fwd_op.register_fake
def _(logits, labels, shift, ignore_index, reduction):
    rows, _, _ = ops.check_ce(logits, labels, shift, ignore_index, reduction)
    return (logits.new_empty((), dtype=torch.float32), logits.new_empty((rows,), dtype=torch.float32),
            logits.new_empty((1,), dtype=torch.int64))


@torch.library.custom_op("llmqat_amd::ce_bwd", mutates_args=(), device_types="cuda")
def ce_bwd_op(logits: torch.Tensor, labels: torch.Tensor, row_lse: torch.Tensor, n_valid: torch.Tensor, grad_loss: torch.Tensor, shift: bool,
              ignore_index: int, reduction: str) -> torch.Tensor:
    return ops.ce_backward(logits, labels, row_lse, n_valid, grad_loss, shift, ignore_index, reduction)


@ce_bwd_op.register_fake
def _(logits, labels, row_lse, n_valid, grad_loss, shift, ignore_index, reduction):
    ops.check_ce(logits, labels, shift, ignore_index, reduction)
    return torch.empty_like(logits, memory_format=torch.contiguous_format)


def _ce_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1], output[2])
    ctx.ce_settings = inputs[2:]


def _ce_backward(ctx, grad_loss, grad_lse, grad_n):
    logits, labels, row_lse, n_valid = ctx.saved_tensors
    return ce_bwd_op(logits, labels, row_lse, n_valid, grad_loss, *ctx.ce_settings), None, None, None, None


ce_fwd_op.register_autograd(_ce_backward, setup_context=_ce_setup)


def ce_loss(logits, labels, shift, ignore_index, reduction):
    """lm_loss.cross_entropy / causal_lm_loss while compiling"""
    return ce_fwd_op(logits, labels, shift, ignore_index, reduction)[0]


# ---- the RMSNorm (ops.rms_norm_forward / ops.rms_norm_backward): (y, rstd) and (dx, dw) ------------------------------
@torch.library.custom_op("llmqat_amd::rms_norm_fwd", mutates_args=(), device_types="cuda")
def rms_norm_fwd_op(x: torch.Tensor, weight: torch.Tensor, eps: float, need_stats: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    y, rstd = ops.rms_norm_forward(x, weight, eps, need_stats)
    return y, (rstd if need_stats else x.new_empty(0, dtype=torch.float32))      # an op returns tensors: an empty one for "not written"


@rms_norm_fwd_op.register_fake
def _(x, weight, eps, need_stats):
    rows, _ = ops.check_rms_norm(x, weight, eps)
    return x.new_empty(x.shape, dtype=weight.dtype), x.new_empty((rows if need_stats else 0,), dtype=torch.float32)


@torch.library.custom_op("llmqat_amd::rms_norm_bwd", mutates_args=(), device_types="cuda")
def rms_norm_bwd_op(g: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, rstd: torch.Tensor, need_dx: bool, need_dw: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    dx, dw = ops.rms_norm_backward(g, x, weight, rstd, need_dx, need_dw)
    return (dx if need_dx else x.new_empty(0)), (dw if need_dw else weight.new_empty(0))      # an op returns tensors: an empty one for "not asked for"


@rms_norm_bwd_op.register_fake
def _(g, x, weight, rstd, need_dx, need_dw):
    ops.check_rms_norm(x, weight)
    return (torch.empty_like(x, memory_format=torch.contiguous_format) if need_dx else x.new_empty(0),
            torch.empty_like(weight) if need_dw else weight.new_empty(0))


def _rms_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1])


def _rms_backward(ctx, grad_y, grad_rstd):
    x, weight, rstd = ctx.saved_tensors
    need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dx, dw = rms_norm_bwd_op(grad_y, x, weight, rstd, need_dx, need_dw)
    return (dx if need_dx else None), (dw if need_dw else None), None, None


rms_norm_fwd_op.register_autograd(_rms_backward, setup_context=_rms_setup)


def rms_norm(x, weight, eps):
    """norm.rms_norm while compiling; as in eager mode no rstd is written when no gradient can be asked for (grad mode and the inputs'
    requires_grad are known while tracing)"""
    need = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)
    return rms_norm_fwd_op(x, weight, float(eps), need)[0]


# ---- the gated activation (ops.swiglu_forward / ops.swiglu_backward): y and (dgate, dup) ----------------------------------
@torch.library.custom_op("llmqat_amd::swiglu_fwd", mutates_args=(), device_types="cuda")
def swiglu_fwd_op(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return ops.swiglu_forward(gate, up)


@swiglu_fwd_op.register_fake
def _(gate, up):
    ops.check_swiglu(gate, up)
    return gate.new_empty(gate.shape)


@torch.library.custom_op("llmqat_amd::swiglu_bwd", mutates_args=(), device_types="cuda")
def swiglu_bwd_op(dy: torch.Tensor, gate: torch.Tensor, up: torch.Tensor, need_dgate: bool, need_dup: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    dgate, dup = ops.swiglu_backward(dy, gate, up, need_dgate, need_dup)
    return (dgate if need_dgate else gate.new_empty(0)), (dup if need_dup else gate.new_empty(0))      # an op returns tensors: an empty one for "not asked for"


@swiglu_bwd_op.register_fake
def _(dy, gate, up, need_dgate, need_dup):
    ops.check_swiglu(gate, up)
    return (gate.new_empty(gate.shape) if need_dgate else gate.new_empty(0)), (gate.new_empty(gate.shape) if need_dup else gate.new_empty(0))


def _swiglu_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])


def _swiglu_backward(ctx, grad_y):
    gate, up = ctx.saved_tensors
    need_dgate, need_dup = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_dgate or need_dup):
        return None, None
    dgate, dup = swiglu_bwd_op(grad_y, gate, up, need_dgate, need_dup)
    return (dgate if need_dgate else None), (dup if need_dup else None)


swiglu_fwd_op.register_autograd(_swiglu_backward, setup_context=_swiglu_setup)


def swiglu(gate, up):
    """mlp.swiglu while compiling"""
    return swiglu_fwd_op(gate, up)


# ---- the rotary embedding (ops.rope_forward / ops.rope_backward): (q_embed, k_embed) and (dq, dk) -----------------------
def _rope_empty(like, shape, strides, dtype):
    return like.new_empty_strided(shape, ops.rope_dense_like(shape, strides), dtype=dtype)


@torch.library.custom_op("llmqat_amd::rope_fwd", mutates_args=(), device_types="cuda")
def rope_fwd_op(q: torch.Tensor, k: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, position_ids: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.rope_forward(q, k, cos, sin, position_ids)


@rope_fwd_op.register_fake
def _(q, k, cos, sin, position_ids):
    ops.check_rope(q, k, cos, sin, position_ids)
    rdt = ops.rope_result_dtype(q.dtype, k.dtype)
    return _rope_empty(q, list(q.shape), list(q.stride()), rdt), _rope_empty(k, list(k.shape), list(k.stride()), rdt)


@torch.library.custom_op("llmqat_amd::rope_bwd", mutates_args=(), device_types="cuda")
def rope_bwd_op(dq_out: torch.Tensor, dk_out: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, position_ids: Optional[torch.Tensor],
                q_shape: List[int], q_strides: List[int], q_dtype: torch.dtype, k_shape: List[int], k_strides: List[int], k_dtype: torch.dtype,
                need_dq: bool, need_dk: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    dq, dk = ops.rope_backward(dq_out, dk_out, cos, sin, position_ids, (q_shape, q_strides, q_dtype), (k_shape, k_strides, k_dtype), need_dq, need_dk)
    return (dq if need_dq else cos.new_empty(0)), (dk if need_dk else cos.new_empty(0))      # an op returns tensors: an empty one for "not asked for"


@rope_bwd_op.register_fake
def _(dq_out, dk_out, cos, sin, position_ids, q_shape, q_strides, q_dtype, k_shape, k_strides, k_dtype, need_dq, need_dk):
    return ((_rope_empty(dq_out, q_shape, q_strides, q_dtype) if need_dq else cos.new_empty(0)),
            (_rope_empty(dk_out, k_shape, k_strides, k_dtype) if need_dk else cos.new_empty(0)))


def _rope_setup(ctx, inputs, output):
    q, k, cos, sin, position_ids = inputs
    ctx.save_for_backward(cos, sin, *(() if position_ids is None else (position_ids,)))       # the tables and positions alone
    ctx.like = (list(q.shape), list(q.stride()), q.dtype, list(k.shape), list(k.stride()), k.dtype)


def _rope_backward(ctx, dq_out, dk_out):
    cos, sin, *pos = ctx.saved_tensors
    need_dq, need_dk = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not (need_dq or need_dk):
        return None, None, None, None, None
    dq, dk = rope_bwd_op(dq_out, dk_out, cos, sin, pos[0] if pos else None, *ctx.like, need_dq, need_dk)
    return (dq if need_dq else None), (dk if need_dk else None), None, None, None


rope_fwd_op.register_autograd(_rope_backward, setup_context=_rope_setup)


def rope(q, k, cos, sin, position_ids=None):
    """rope.rotary while compiling (a tensor whose last stride is not 1 is copied in front of the op, so that the op's results have the
    layout its fake implementation states)"""
    q, k = (t if t.stride(-1) == 1 else t.contiguous() for t in (q, k))
    return rope_fwd_op(q, k, cos, sin, position_ids)


# ---- the attention softmax (ops.attn_softmax_forward / ops.attn_softmax_backward): (y, stats) and dx ------------------
@torch.library.custom_op("llmqat_amd::attn_softmax_fwd", mutates_args=(), device_types="cuda")
def attn_softmax_fwd_op(scores: torch.Tensor, mask: Optional[torch.Tensor], inv: float, need_stats: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    y, stats = ops.attn_softmax_forward(scores, mask, scale=inv, need_stats=need_stats)
    return y, (stats if need_stats else scores.new_empty((0, 2), dtype=torch.float32))      # an op returns tensors: an empty one for "not written"


@attn_softmax_fwd_op.register_fake
def _(scores, mask, inv, need_stats):
    B, H, T, _, _ = ops.check_attn_softmax(scores, mask, scale=inv)
    return torch.empty_like(scores, memory_format=torch.contiguous_format), scores.new_empty((B * H * T if need_stats else 0, 2), dtype=torch.float32)


@torch.library.custom_op("llmqat_amd::attn_softmax_bwd", mutates_args=(), device_types="cuda")
def attn_softmax_bwd_op(g: torch.Tensor, scores: torch.Tensor, mask: Optional[torch.Tensor], stats: torch.Tensor, inv: float) -> torch.Tensor:
    return ops.attn_softmax_backward(g, scores, mask, stats, scale=inv)


@attn_softmax_bwd_op.register_fake
def _(g, scores, mask, stats, inv):
    ops.check_attn_softmax(scores, mask, scale=inv)
    return torch.empty_like(scores, memory_format=torch.contiguous_format)


def _attn_setup(ctx, inputs, output):
    scores, mask, inv, _ = inputs
    ctx.save_for_backward(scores, output[1], *(() if mask is None else (mask,)))       # the scores, the stats and the mask alone
    ctx.inv = inv


def _attn_backward(ctx, grad_y, grad_stats):
    scores, stats, *mask = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None
    return attn_softmax_bwd_op(grad_y, scores, mask[0] if mask else None, stats, ctx.inv), None, None, None


attn_softmax_fwd_op.register_autograd(_attn_backward, setup_context=_attn_setup)


def attn_softmax(scores, mask, inv):
    """attention.attn_softmax while compiling; as in eager mode no stats are written when no gradient can be asked for"""
    need = torch.is_grad_enabled() and scores.requires_grad
    return attn_softmax_fwd_op(scores, mask, inv, need)[0]
