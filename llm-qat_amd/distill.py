"""The distillation loss an LLM-QAT step ends with (the reference's utils/kd_trainer.py:42-48), fused:

    F.kl_div(F.log_softmax(student_logits, dim=-1), F.softmax(teacher_logits, dim=-1), reduction="batchmean")

as one forward and one backward HIP kernel pass over the logits instead of an eager chain of fp32 [rows, vocabulary] temporaries.

    from llm_qat_amd.distill import kd_kl_loss, install
    loss = kd_kl_loss(student_logits, teacher_logits.detach())
    previous = install(KDTrainer)          # KDTrainer.ce_loss now runs kd_kl_loss; no edit of the trainer
"""
import torch

from . import compiled, cpu_tensors, ops

__all__ = ["kd_kl_loss", "install"]


def _cpu_rows(s, t):
    """the contract's formula in torch ops, fp32, on [rows, cols] views, each row taken relative to its maximum as the kernels do
    -> (s - max s, t - max t, log sum e^(s - max s), log sum e^(t - max t)) with the row dimension kept; a row of only -inf: max 0"""
    def rel(x):
        m = x.amax(dim=-1, keepdim=True)
        d = x - torch.where(m == float("-inf"), torch.zeros_like(m), m)
        return d, torch.log(torch.exp(d).sum(-1, keepdim=True, dtype=torch.float64)).float()      # fp32 terms, summed in float64
    return rel(s) + rel(t)


class _KDKLCpu(torch.autograd.Function):
    """CPU tensors (opt-in, cpu_tensors.py): selected by the tensors' device, never a fallback of the CUDA path"""

    @staticmethod
    def forward(ctx, student, teacher):
        cols, batch = student.shape[-1], student.shape[0]
        s, t = student.detach().reshape(-1, cols).float(), teacher.detach().reshape(-1, cols).float()
        ds, ls, dt, lt = _cpu_rows(s, t)
        p_t = torch.exp(dt - lt)
        term = torch.where(p_t == 0, torch.zeros_like(p_t), p_t * (dt - ds))     # p_t == 0 contributes 0, also under s = -inf
        ctx.save_for_backward(student, teacher)
        return (((term.sum(-1, keepdim=True, dtype=torch.float64) - lt) + ls).sum() / batch).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_loss):
        student, teacher = ctx.saved_tensors
        cols, batch = student.shape[-1], student.shape[0]
        s, t = student.reshape(-1, cols).float(), teacher.reshape(-1, cols).float()
        ds, ls, dt, lt = _cpu_rows(s, t)
        grad = (grad_loss.float() / batch) * (torch.exp(ds - ls) - torch.exp(dt - lt))
        return grad.to(student.dtype).reshape(student.shape), None


class _KDKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, need):
        student, teacher, _, _, _ = ops.kd_inputs(student.detach(), teacher.detach())
        loss, row_stats, _ = ops.kd_kl_forward(student, teacher, need_stats=need)     # no gradient wanted: no stats buffer
        if need:
            ctx.save_for_backward(student, teacher, row_stats)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        student, teacher, row_stats = ctx.saved_tensors
        return ops.kd_kl_backward(student, teacher, row_stats, grad_loss), None, None


def kd_kl_loss(student_logits, teacher_logits):
    """kl_div(log_softmax(student_logits, -1), softmax(teacher_logits, -1), reduction="batchmean"): the sum over every position and
    vocabulary entry of p_t (log p_t - log p_s), divided by shape[0] (the batch, not the row count).  -> an fp32 0-dim tensor whose
    gradient for student_logits is (g / shape[0]) (softmax(student) - softmax(teacher)) in student_logits' dtype, rounded once from fp32.

    Both logits: the same shape [batch, ..., vocabulary] (two dimensions or more), the same dtype (float32, bfloat16 or float16), the
    same CUDA device; a non-contiguous one is copied once.  The teacher has no gradient: a teacher that requires grad is refused.

    Arithmetic is fp32 whatever the dtype, which is what the reference's chain computes under CUDA autocast (softmax, log_softmax and
    kl_div are fp32 ops there).  OUTSIDE autocast the reference computes 16-bit logits in 16 bits and returns a 16-bit loss; this
    function does not follow that: it returns the fp32 result.  Agreement with the chain is to rounding error (measured against
    float64, tests/kd_loss_reference.py), not bit for bit.  kd_kl_loss(s, s.detach()) is exactly 0.0 with an all-zero gradient.  An
    element that is -inf in both tensors contributes 0 (the reference: NaN); a student -inf under a teacher probability > 0 gives +inf;
    a NaN makes its row's loss and gradient, and the total, NaN.  No temperature, no masking, no log_target, as the reference has none.

    CPU tensors are refused unless llm_qat_amd.allow_cpu_tensors(True): then the same formula runs in torch ops, fp32."""
    ops.check_kd(student_logits, teacher_logits)
    if student_logits.device.type == "cpu" and teacher_logits.device.type == "cpu":
        if not cpu_tensors.ENABLED:
            cpu_tensors.refuse(student_logits, "kd_kl_loss")
        return _KDKLCpu.apply(student_logits, teacher_logits)
    if torch.compiler.is_compiling():
        return compiled.kd_kl_loss(student_logits, teacher_logits)
    need = torch.is_grad_enabled() and student_logits.requires_grad      # no backward will come: no stats buffer is written
    return _KDKL.apply(student_logits, teacher_logits, need)


def install(trainer_cls):
    """Replace trainer_cls.ce_loss (the reference's KDTrainer: `ce_loss(self, size_average, student_logits, teacher_logits)`) with a
    method of that signature that returns kd_kl_loss(student_logits, teacher_logits).  size_average is ignored, as the reference's method
    ignores it.  -> the previous method (None if the class had none): assign it back to undo."""
    if not isinstance(trainer_cls, type):
        raise TypeError(f"install: expected a class (the KDTrainer), got {type(trainer_cls).__name__}")
    previous = trainer_cls.__dict__.get("ce_loss", getattr(trainer_cls, "ce_loss", None))

    def ce_loss(self, size_average, student_logits, teacher_logits):
        return kd_kl_loss(student_logits, teacher_logits)

    trainer_cls.ce_loss = ce_loss
    return previous
