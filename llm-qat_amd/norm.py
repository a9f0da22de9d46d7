"""The RMSNorm of a LLaMA decoder (the reference's LlamaRMSNorm, models/modeling_llama_quant.py:112-129), fused:

    variance      = hidden_states.to(torch.float32).pow(2).mean(-1, keepdim=True)
    hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
    if self.weight.dtype in [torch.float16, torch.bfloat16]:
        hidden_states = hidden_states.to(self.weight.dtype)
    return self.weight * hidden_states

as one forward HIP kernel and a two-launch backward: no fp32 [rows, hidden] temporary, and nothing saved but x, the weight and one fp32
per row.

    from llm_qat_amd.norm import RMSNorm, convert, install, rms_norm
    previous = install(models.modeling_llama_quant)    # no edit: models built from now on use the fused class
    convert(teacher)                                   # an existing model (stock Hugging Face norms too), in place
"""
import torch

from . import compiled, cpu_tensors, ops

__all__ = ["rms_norm", "RMSNorm", "install", "convert"]


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps, need):
        xc, wc, _, _ = ops.rms_norm_inputs(x.detach(), weight.detach(), eps)
        y, rstd = ops.rms_norm_forward(xc, wc, eps, need_stats=need)      # no gradient can be asked for: no stats
        if need:
            ctx.save_for_backward(xc, wc, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, rstd = ctx.saved_tensors
        dx, dw = ops.rms_norm_backward(g, x, weight, rstd, ctx.needs_input_grad[0], ctx.needs_input_grad[1])   # a frozen weight: no dw stage
        return dx, dw, None, None


def rms_norm(x, weight, eps=1e-6):
    """weight * (x * rsqrt(mean(x^2, -1) + eps)) as LlamaRMSNorm.forward computes it: fp32 arithmetic in the chain's op order with its
    roundings, the result in the weight's dtype.  Given the same rsqrt the result equals the chain's bit for bit; the sum of squares runs
    in another order than ATen's, so the last bit of a row's rsqrt, and through it a small share of that row's elements, can differ
    (DESIGN.md section 25 has the bound).  The gradients are the fp32 formulas of the unrounded function (the casts count as the
    identity, as autograd counts them), each rounded once: x's in x's dtype, the weight's in the weight's.

    x: [..., hidden], weight: [hidden]; float32, bfloat16 or float16, equal or exactly one of the two float32; on a CUDA device; a
    non-contiguous x is copied once.  A weight that does not require grad launches nothing for its gradient; under no_grad no statistic
    is written.  A NaN stays in its row.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the reference's lines
    run in torch ops."""
    ops.check_rms_norm(x, weight, eps, "rms_norm")
    if x.device.type == "cpu" and weight.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(x, "rms_norm")
        return cpu_tensors.rms_norm(x, weight, eps)
    if torch.compiler.is_compiling():
        return compiled.rms_norm(x, weight, eps)
    need = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)
    return _RMSNorm.apply(x, weight, eps, need)


class RMSNorm(torch.nn.Module):
    """LlamaRMSNorm's constructor, attributes (weight, variance_epsilon) and state_dict: checkpoints load either way."""

    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def extra_repr(self):
        return f"{self.weight.shape[0]}, eps={self.variance_epsilon}"

    def forward(self, hidden_states):
        return rms_norm(hidden_states, self.weight, self.variance_epsilon)


def install(namespace):
    """Replace the attribute LlamaRMSNorm of a module object (the reference's models.modeling_llama_quant, whose decoder layers and
    model look the class up when they are built) with this module's class.  -> the previous attribute (None if there was none): assign
    it back to undo.  Models built before the call keep their norms: convert() swaps those."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    previous = getattr(namespace, "LlamaRMSNorm", None)
    namespace.LlamaRMSNorm = RMSNorm
    return previous


def _is_rms_norm(m):
    w = getattr(m, "weight", None)
    return (not isinstance(m, RMSNorm) and isinstance(w, torch.nn.Parameter) and w.dim() == 1 and hasattr(m, "variance_epsilon")
            and getattr(m, "bias", None) is None)


def convert(model):
    """Swap, in place, every submodule of `model` that has a 1-D `weight` parameter and a `variance_epsilon` attribute (the reference's
    LlamaRMSNorm, Hugging Face's stock one) and is not an RMSNorm already for an RMSNorm over the SAME Parameter object (optimizers and
    tied references stay valid).  -> the number replaced.  `model` itself is not swapped: pass its parent."""
    if not isinstance(model, torch.nn.Module):
        raise TypeError(f"convert: expected a torch.nn.Module, got {type(model).__name__}")
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if _is_rms_norm(child):
                new = RMSNorm(1, child.variance_epsilon)
                new.weight = child.weight
                new.train(child.training)
                setattr(parent, name, new)
                n += 1
    return n
