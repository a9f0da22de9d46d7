"""The language-model loss inside a causal LM's own forward (the reference's models/modeling_llama_quant.py:885-895), fused (DESIGN.md
section 23):

    shift_logits = logits[..., :-1, :].contiguous()
    shift_labels = labels[..., 1:].contiguous()
    loss = CrossEntropyLoss()(shift_logits.view(-1, V), shift_labels.view(-1))

as one forward and one backward HIP kernel pass over the unshifted logits: no [B, T-1, V] copy, no fp32 cast, no fp32 log-softmax.

    from llm_qat_amd.lm_loss import causal_lm_loss, install
    loss = causal_lm_loss(logits, labels)              # the one-line edit: the three lines above, the shift done in the kernel
    previous = install(models.modeling_llama_quant)    # no edit: the module's CrossEntropyLoss is the fused one (the shift copy stays)
"""
import torch

from . import compiled, cpu_tensors, ops

__all__ = ["cross_entropy", "causal_lm_loss", "CrossEntropyLoss", "install"]

_SERVED = ("llm_qat_amd.lm_loss serves int64 class-index targets with ignore_index and reduction 'mean' or 'sum', which is what the "
           "reference's language-model loss uses")


def _effective_labels(labels, shift, ignore_index):
    """[rows] labels as the kernels see them: with shift, row r takes labels[r + 1] and the last position of a sequence is ignored"""
    if not shift:
        return labels.reshape(-1)
    last = labels.new_full(labels.shape[:-1] + (1,), ignore_index)
    return torch.cat([labels[..., 1:], last], dim=-1).reshape(-1)


def _cpu_rows(logits, labels, shift, ignore_index):
    """the contract's formula in torch ops on [rows, cols], in float64 (the results are rounded once, to fp32 and to the logits' dtype)
    -> (x, y clamped into the row, valid, lse) with lse = NaN for a valid row whose label lies outside [0, cols); ignored rows are
    masked out of every result, whatever they hold"""
    cols = logits.shape[-1]
    x = logits.detach().reshape(-1, cols).double()
    y = _effective_labels(labels, shift, ignore_index)
    valid = y != ignore_index
    x = torch.where(valid.unsqueeze(-1), x, torch.zeros_like(x))
    m = x.amax(dim=-1, keepdim=True)
    m = torch.where(m == float("-inf"), torch.zeros_like(m), m)
    lse = (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))).squeeze(-1)
    in_range = (y >= 0) & (y < cols)
    lse = torch.where(in_range | ~valid, lse, torch.full_like(lse, float("nan")))
    return x, y.clamp(0, cols - 1), valid, lse


class _CECpu(torch.autograd.Function):
    """CPU tensors (opt-in, cpu_tensors.py): selected by the tensors' device, never a fallback of the CUDA path"""

    @staticmethod
    def forward(ctx, logits, labels, shift, ignore_index, reduction):
        x, y, valid, lse = _cpu_rows(logits, labels, shift, ignore_index)
        row_loss = torch.where(valid, lse - x.gather(1, y.unsqueeze(1)).squeeze(1), torch.zeros_like(lse))
        total = row_loss.sum()
        ctx.save_for_backward(logits, labels)
        ctx.settings = (shift, ignore_index, reduction)
        return (total / valid.sum() if reduction == "mean" else total).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_loss):
        logits, labels = ctx.saved_tensors
        shift, ignore_index, reduction = ctx.settings
        x, y, valid, lse = _cpu_rows(logits, labels, shift, ignore_index)
        p = torch.exp(x - lse.unsqueeze(-1))
        p.scatter_add_(1, y.unsqueeze(1), -torch.ones_like(lse).unsqueeze(1))
        gn = grad_loss.double() / valid.sum() if reduction == "mean" else grad_loss.double()
        grad = torch.where(valid.unsqueeze(-1), gn * p, torch.zeros_like(p))
        return grad.to(logits.dtype).reshape(logits.shape), None, None, None, None


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, shift, ignore_index, reduction, need):
        logits, labels, _, _, _ = ops.ce_inputs(logits.detach(), labels, shift, ignore_index, reduction)
        loss, row_lse, _, n_valid = ops.ce_forward(logits, labels, shift, ignore_index, reduction, need_stats=need)   # no gradient wanted: no stats
        if need:
            ctx.save_for_backward(logits, labels, row_lse, n_valid)
            ctx.settings = (shift, ignore_index, reduction)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, labels, row_lse, n_valid = ctx.saved_tensors
        return ops.ce_backward(logits, labels, row_lse, n_valid, grad_loss, *ctx.settings), None, None, None, None, None


def _loss(logits, labels, shift, ignore_index, reduction, what):
    ops.check_ce(logits, labels, shift, ignore_index, reduction, what)
    if logits.device.type == "cpu" and labels.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(logits, what)
        return _CECpu.apply(logits, labels, shift, ignore_index, reduction)
    if torch.compiler.is_compiling():
        return compiled.ce_loss(logits, labels, shift, ignore_index, reduction)
    need = torch.is_grad_enabled() and logits.requires_grad      # no backward will come: no stats buffer is written
    return _CE.apply(logits, labels, shift, ignore_index, reduction, need)


def cross_entropy(logits, target, ignore_index=-100, reduction="mean"):
    """F.cross_entropy(logits, target, ignore_index=, reduction=) for class-index targets: with lse_r = logsumexp(logits[r]) and the valid
    rows those whose target is not ignore_index (n of them), the mean ("mean") or the sum ("sum") over the valid rows of
    lse_r - logits[r, target[r]].  -> an fp32 0-dim tensor whose gradient for the logits is (g / n) (softmax(logits) - onehot(target)) on
    valid rows (the divisor is 1 under "sum") and zero on ignored ones, in the logits' dtype, rounded once from fp32.

    logits: [N, V] (or [..., V] with target [...]), float32, bfloat16 or float16, on a CUDA device; target: int64, same device; a
    non-contiguous tensor is copied once.  "mean" over no valid row is NaN, as ATen's; "sum" is 0.

    Arithmetic is fp32 whatever the dtype, which is what F.cross_entropy computes under CUDA autocast (it is an fp32-cast op there).
    OUTSIDE autocast the reference computes 16-bit logits in 16 bits and returns a 16-bit loss; this function does not follow that: it
    returns the fp32 result.  Agreement with ATen is to rounding error (measured against float64, tests/ce_loss_reference.py), not bit
    for bit.  An ignored row is never read: a NaN or inf there reaches neither the loss nor any gradient (ATen's backward gives NaN in
    that row: the one documented deviation).  A NaN in a valid row makes that row's gradient and the loss NaN, and no other row's
    gradient.  A target outside [0, V) that is not ignore_index is never used as an address: its row counts as valid, and the loss and
    that row's gradient are NaN (ATen asserts on the device).  Class weights, label smoothing, probability targets and
    reduction="none" are not served, as the reference uses none of them.

    CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the same formula runs in torch ops, in float64, rounded once."""
    return _loss(logits, target, False, ignore_index, reduction, "cross_entropy")


def causal_lm_loss(logits, labels, ignore_index=-100, reduction="mean"):
    """The loss of a causal language model on logits [..., T, V] and labels [..., T]: position t is scored against labels[t + 1],

        cross_entropy(logits[..., :-1, :].reshape(-1, V), labels[..., 1:].reshape(-1), ignore_index, reduction)

    with the shift done inside the kernels, on the unshifted contiguous tensors: no [..., T-1, V] copy exists.  The gradient is the full
    [..., T, V] tensor, all-zero at the last position of every sequence (which is never read).  Everything else as cross_entropy: fp32
    arithmetic whatever the dtype (what the reference's lines compute under the CUDA autocast it trains with; outside autocast they
    compute 16-bit logits in 16 bits, which this function does not follow), an fp32 0-dim loss, ignored rows never read."""
    return _loss(logits, labels, True, ignore_index, reduction, "causal_lm_loss")


class CrossEntropyLoss(torch.nn.Module):
    """torch.nn.CrossEntropyLoss's constructor, serving what the reference's language-model loss uses: forward(input [N, V], target [N])
    is cross_entropy(input, target, ignore_index, reduction).  Refused at construction: weight, label_smoothing != 0, the legacy
    size_average / reduce, reduction="none"."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError(f"CrossEntropyLoss: class weights are not served. {_SERVED}")
        if size_average is not None or reduce is not None:
            raise NotImplementedError(f"CrossEntropyLoss: the legacy size_average / reduce arguments are not served; pass reduction=. {_SERVED}")
        if label_smoothing != 0:
            raise NotImplementedError(f"CrossEntropyLoss: label_smoothing={label_smoothing} is not served. {_SERVED}")
        if reduction not in ("mean", "sum"):
            raise NotImplementedError(f"CrossEntropyLoss: reduction={reduction!r} is not served. {_SERVED}")
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
            raise TypeError(f"CrossEntropyLoss: ignore_index is an int, got {type(ignore_index).__name__}")
        self.ignore_index = ignore_index
        self.reduction = reduction

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}, reduction={self.reduction!r}"

    def forward(self, input, target):
        return cross_entropy(input, target, self.ignore_index, self.reduction)


def install(namespace):
    """Replace the attribute CrossEntropyLoss of a module object (the reference's models.modeling_llama_quant, which does
    `from torch.nn import CrossEntropyLoss` and builds one in every forward) with this module's class.  -> the previous attribute (None
    if there was none): assign it back to undo.  The model's own shift copy stays; causal_lm_loss is the one-line edit that removes it."""
    import types
    if not isinstance(namespace, types.ModuleType):
        raise TypeError(f"install: expected a module object (e.g. models.modeling_llama_quant), got {type(namespace).__name__}")
    previous = getattr(namespace, "CrossEntropyLoss", None)
    namespace.CrossEntropyLoss = CrossEntropyLoss
    return previous
