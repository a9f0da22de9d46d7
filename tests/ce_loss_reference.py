"""Reference, error measures, case list and caps for the fused language-model loss (llm_qat_amd.lm_loss).

The bar is error against float64, measured beside the eager fp32 chain's own error: bit parity with ATen is not on offer for a reduction
over the vocabulary in another order.  Both measures are in units of 2^-24 (fp32's unit roundoff).

  E_loss(x) = |x - loss64| / N,   N = sum over valid rows of (|lse_r| + |x_r[y_r]|) / n
      A row's loss is the difference lse_r - x_r[y_r], so an error relative to the loss itself would be ill-conditioned; N is the
      magnitude of what is subtracted and added up (n = 1 in the divisor under reduction="sum").
  C_grad(x) = max over the elements of valid rows of (|x - d64| - u |d64| - A)+ / ((p + onehot) |g| / n)
      u: the one output rounding (0 for fp32, 2^-8 for bf16, 2^-11 for fp16); A: flush to zero and subnormals (2^-120; 2^-25 for
      fp16): the U_OUT / A_OUT of tests/kd_loss_reference.py.

LOSS_CAP and GRAD_CAP are 4 x the eager chain's largest measure over CASES on the MI355X: a factor 2 for hardware exp / log with the
x * log2(e) prescale against ATen's functions, times 2 for another summation order.  They come from the eager chain, never from the kernels.
"""
import torch
import torch.nn.functional as F

from kd_loss_reference import A_OUT, U_OUT, UNIT

IGNORE = -100

# The eager chain's largest measures over CASES, as measured by eager_measures() (fp32 inputs, fp32 gradient):
#   on the MI355X (ROCm's ATen kernels):  E_loss 0.9950 (randn_s6_v4099), C_grad 60.50 (randn_s30_v33)    <- what the caps are made of
#   on the CPU (ATen's CPU kernels):      E_loss 0.781 (randn_s1_v4099), C_grad 60.50 (randn_s30_v33)
# The fused path runs on the MI355X, so its bar is the chain it replaces there.  (The fused path itself: 1.51 and 92.1 at most.)
EAGER_E_LOSS = 0.996
EAGER_C_GRAD = 60.6
LOSS_CAP = 4 * EAGER_E_LOSS
GRAD_CAP = 4 * EAGER_C_GRAD


def chain(logits, labels):
    """the reference's three lines (models/modeling_llama_quant.py:885-895) on [..., T, V] logits and [..., T] labels"""
    v = logits.shape[-1]
    return F.cross_entropy(logits[..., :-1, :].contiguous().view(-1, v), labels[..., 1:].contiguous().view(-1))


def ref64(x, y, reduction="mean", ignore_index=IGNORE):
    """F.cross_entropy on [rows, V] logits and [rows] labels in float64 with autograd
    -> loss64, d64 (upstream gradient 1), lse, xy = x[r, y_r], p = softmax, onehot, valid (float64 / bool, on x's device)"""
    x64 = x.detach().double().requires_grad_(True)
    loss = F.cross_entropy(x64, y, ignore_index=ignore_index, reduction=reduction)
    (d,) = torch.autograd.grad(loss, x64)
    x64 = x64.detach()
    valid = y != ignore_index
    lse = torch.logsumexp(x64, dim=-1)
    yc = torch.where(valid, y, torch.zeros_like(y))
    xy = x64.gather(1, yc.unsqueeze(1)).squeeze(1)
    onehot = torch.zeros_like(x64).scatter_(1, yc.unsqueeze(1), 1.0) * valid.unsqueeze(1)
    return loss.detach(), d, lse, xy, torch.exp(x64 - lse.unsqueeze(-1)), onehot, valid


def eager32(x, y, reduction="mean", ignore_index=IGNORE):
    """F.cross_entropy on .float() inputs, which is what CUDA autocast runs -> loss32, d32 (fp32)"""
    x32 = x.detach().float().requires_grad_(True)
    loss = F.cross_entropy(x32, y, ignore_index=ignore_index, reduction=reduction)
    (d,) = torch.autograd.grad(loss, x32)
    return loss.detach(), d


def effective_labels(labels, shift, ignore_index=IGNORE):
    """the contract's effective label of every row, [rows]: with shift, labels[r + 1], and the last position of a sequence ignored"""
    if not shift:
        return labels.reshape(-1)
    return torch.cat([labels[..., 1:], labels.new_full(labels.shape[:-1] + (1,), ignore_index)], dim=-1).reshape(-1)


def formula64(logits, labels, shift=False, reduction="mean", ignore_index=IGNORE):
    """the contract in float64, written out -> loss, grad (of the logits' shape), row_loss, n; ignored rows are never looked at"""
    v = logits.shape[-1]
    x = logits.detach().double().reshape(-1, v)
    y = effective_labels(labels, shift, ignore_index)
    valid = y != ignore_index
    n = int(valid.sum())
    row_loss, grad = torch.zeros(x.shape[0], dtype=torch.float64), torch.zeros_like(x)
    div = n if reduction == "mean" else 1
    for r in range(x.shape[0]):
        if valid[r]:
            lse = torch.logsumexp(x[r], dim=-1)
            row_loss[r] = lse - x[r, y[r]]
            grad[r] = torch.exp(x[r] - lse)
            grad[r, y[r]] -= 1.0
            grad[r] /= div if div else float("nan")
    total = row_loss.sum()
    loss = (total / n if n else torch.tensor(float("nan"), dtype=torch.float64)) if reduction == "mean" else total
    return loss, grad.reshape(logits.shape), row_loss, n


def _div(valid, reduction):
    return int(valid.sum()) if reduction == "mean" else 1


def e_loss(loss, x, y, reduction="mean", ref=None):
    loss64, _, lse, xy, _, _, valid = ref or ref64(x, y, reduction)
    n = ((lse.abs() + xy.abs()) * valid).sum() / _div(valid, reduction)
    return float((loss.detach().double().to(loss64.device) - loss64).abs() / n / UNIT)


def c_grad(grad, x, y, dtype=torch.float32, g=1.0, reduction="mean", ref=None, n=None):
    """n: the divisor d64 was made with, where `ref` holds only some of the rows it counted"""
    _, d64, _, _, p, onehot, valid = ref or ref64(x, y, reduction)
    d64 = d64 * g
    num = ((grad.detach().double().to(d64.device) - d64).abs() - U_OUT[dtype] * d64.abs() - A_OUT[dtype]).clamp_min(0)
    den = (p + onehot) * abs(g) / (n or _div(valid, reduction))
    q = torch.where(num == 0, torch.zeros_like(num), num / den)        # 0 / 0 where the probability underflows: no error, no measure
    return float(q[valid].max() / UNIT)


def _case(rows, v, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    # bf16-representable values, so that every dtype of the GPU tier but fp16's range limit sees the inputs the caps were measured on
    x = (torch.randn((rows, v), generator=g) * sigma).bfloat16().float()
    y = torch.randint(0, v, (rows,), generator=g)
    y[2::4] = IGNORE                                   # a quarter of the rows
    return x, y


def cases():
    """name -> (x, y): fp32 [rows, V] logits and int64 [rows] labels on the CPU"""
    out = {}
    for sigma in (1, 3, 6):
        for v in (4099, 32000):
            out[f"randn_s{sigma}_v{v}"] = _case(8, v, float(sigma), 100 * sigma + v)
    out["randn_s30_v33"] = _case(8, 33, 30.0, 33)
    return out


_CASES = None


def CASES():
    """the case list, built once and shared; callers leave the tensors unchanged"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def eager_measures(device="cpu"):
    """name -> (E_loss, C_grad) of the eager fp32 chain on `device`: what the caps are made of"""
    out = {}
    for name, (x, y) in CASES().items():
        x, y = x.to(device), y.to(device)
        ref = ref64(x, y)
        loss, d = eager32(x, y)
        out[name] = (e_loss(loss, x, y, ref=ref), c_grad(d, x, y, ref=ref))
    return out
