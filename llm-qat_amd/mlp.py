"""The middle of a LLaMA MLP (the reference's LlamaMLP.forward, models/modeling_llama_quant.py:234-235), fused:

    self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))

act_fn(gate) * up with act_fn = SiLU becomes one forward HIP kernel and one backward HIP kernel that give the eager chain's bits: nothing
saved but gate and up (the chain also keeps silu(gate)), 6 bytes an element moved forward and 10 backward on bf16 instead of 10 and 18.

    from llm_qat_amd.mlp import SwiGLUMLP, convert, install, swiglu
    previous = install(models.modeling_llama_quant)    # no edit: models built from now on use the fused forward
    convert(teacher)                                   # an existing model (stock Hugging Face MLPs too), in place
"""
import torch

from . import _act_node, compiled, cpu_tensors, ops

__all__ = ["swiglu", "SwiGLUMLP", "install", "convert"]


class _SwiGLU(torch.autograd.Function):
    """the node in Python: serves where the C++ node (_act_node.py) is not built or switched off, and states what that one does"""

    @staticmethod
    def forward(ctx, gate, up, rows, cols, need):
        y, g, u = ops.swiglu_launch_forward(gate, up, rows, cols)
        if need:                                         # no gradient can be asked for: nothing saved
            ctx.save_for_backward(g, u)
            ctx.checked = (rows, cols)
        return y

    @staticmethod
    def backward(ctx, dy):
        need_dgate, need_dup = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_dgate or need_dup):
            return None, None, None, None, None
        gate, up = ctx.saved_tensors
        dgate, dup = ops.swiglu_backward(dy, gate, up, need_dgate, need_dup, ctx.checked)      # a frozen side: neither computed nor stored
        return dgate, dup, None, None, None


def swiglu(gate, up):
    """silu(gate) * up as the eager chain F.silu(gate) * up computes it, forward and backward, bit for bit: fp32 arithmetic in ATen's op
    order with the chain's roundings (silu's output and mul's gradient are rounded to the dtype as the chain stores them).

    gate, up: equal shapes, dtypes (float32, bfloat16 or float16) and devices: no broadcasting, no promotion; on a CUDA device.  A tensor
    whose last stride is 1 and whose rows lie one row stride apart (the halves of gate_up.chunk(2, -1)) is read where it lies; any other
    layout is copied once.  The result is contiguous.  Only gate and up are saved, and nothing under no_grad; a side that does not require
    grad gets no gradient computed.  CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the chain runs in torch ops."""
    rows, cols = ops.check_swiglu(gate, up, "swiglu")
    if gate.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(gate, "swiglu")
        return cpu_tensors.swiglu(gate, up)
    if torch.compiler.is_compiling():
        return compiled.swiglu(gate, up)
    need = torch.is_grad_enabled() and (gate.requires_grad or up.requires_grad)
    node = _act_node.load()
    if node is not None and gate.device.type == "cuda":      # the C++ node: the same launches without Python in front of them
        return node.swiglu(gate, up, rows, cols, need)
    return _SwiGLU.apply(gate, up, rows, cols, need)


class SwiGLUMLP(torch.nn.Module):
    """LlamaMLP's forward over the three given projection modules, which it holds under LlamaMLP's names: the state_dict keys are the same
    and checkpoints load either way."""

    def __init__(self, gate_proj, up_proj, down_proj):
        super().__init__()
        self.gate_proj = gate_proj
        self.up_proj = up_proj
        self.down_proj = down_proj

    def forward(self, x):
        return self.down_proj(swiglu(self.gate_proj(x), self.up_proj(x)))


def _is_silu(act):
    return isinstance(act, torch.nn.SiLU) or act is torch.nn.functional.silu or type(act).__name__ == "SiLUActivation"


def install(namespace):
    """Replace the attribute LlamaMLP of a module object (the reference's models.modeling_llama_quant, whose decoder layers look the
    class up when they are built) with a subclass of it: the constructor and the parameters are the parent's, the forward runs swiglu
    where act_fn is SiLU and is the parent's otherwise.  -> the previous attribute: assign it back to undo.  Models built before the
    call keep their MLPs: convert() swaps those."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    previous = namespace.LlamaMLP

    class LlamaMLP(previous):
        fused_swiglu = True

        def forward(self, x):
            if not _is_silu(getattr(self, "act_fn", None)):
                return super().forward(x)
            return self.down_proj(swiglu(self.gate_proj(x), self.up_proj(x)))

    LlamaMLP.__qualname__ = LlamaMLP.__name__ = getattr(previous, "__name__", "LlamaMLP")
    LlamaMLP.__module__ = getattr(previous, "__module__", LlamaMLP.__module__)
    namespace.LlamaMLP = LlamaMLP
    return previous


def _is_swiglu_mlp(m):
    return (not isinstance(m, SwiGLUMLP) and not getattr(m, "fused_swiglu", False) and _is_silu(getattr(m, "act_fn", None))
            and all(isinstance(getattr(m, n, None), torch.nn.Module) for n in ("gate_proj", "up_proj", "down_proj")))


def convert(model):
    """Swap, in place, every submodule of `model` that has gate_proj, up_proj, down_proj and a SiLU act_fn (torch.nn.SiLU, F.silu, or an
    object of a class named SiLUActivation) and is not converted already for a SwiGLUMLP over the SAME three child modules (parameters,
    optimizers and state_dict keys stay valid).  MLPs with another activation are left alone.  -> the number replaced.  `model` itself
    is not swapped: pass its parent."""
    if not isinstance(model, torch.nn.Module):
        raise TypeError(f"convert: expected a torch.nn.Module, got {type(model).__name__}")
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if _is_swiglu_mlp(child):
                new = SwiGLUMLP(child.gate_proj, child.up_proj, child.down_proj)
                new.train(child.training)
                setattr(parent, name, new)
                n += 1
    return n
