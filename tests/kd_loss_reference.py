"""Reference, error measures, case list and caps for the fused distillation loss (llm_qat_amd.distill).

The bar is error against float64, measured beside the eager fp32 chain's own error: bit parity with ATen is not on offer for a reduction
over the vocabulary in another order.  Both measures are in units of 2^-24 (fp32's unit roundoff).

  E_loss(x) = |x - loss64| / N,   N = (sum |lse_s| + sum |lse_t| + sum p_t |t - s|) / B
      The loss is a cancelling difference of logsumexp values, so an error relative to the loss itself would be ill-conditioned; N is
      the magnitude of what is added up.
  C_grad(x) = max over elements of (|x - ds64| - u |ds64| - A)+ / ((p_s + p_t) |g| / B)
      u: the one output rounding (0 for fp32, 2^-8 for bf16, 2^-11 for fp16); A: flush to zero and subnormals (2^-120; 2^-25 for fp16).
      No ulp distance on 16-bit gradients: the eager chain itself is 2 bf16 ulp off on one case, and 32768 "ulp" off wherever a tiny
      gradient changes sign across zero.

LOSS_CAP and GRAD_CAP are 4 x the eager chain's largest measure over CASES on the MI355X: a factor 2 for hardware exp / log with the x * log2(e)
prescale against ATen's functions, times 2 for another summation order.  They come from the eager chain, never from the kernels.
"""
import torch
import torch.nn.functional as F

UNIT = 2.0 ** -24
U_OUT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
A_OUT = {torch.float32: 2.0 ** -120, torch.bfloat16: 2.0 ** -120, torch.float16: 2.0 ** -25}

# The eager chain's largest measures over CASES, as measured by eager_measures() (fp32 inputs, fp32 gradient):
#   on the MI355X (ROCm's ATen kernels):  E_loss 0.5969 (ramp_v2049), C_grad 50.18 (randn_s30_v33)    <- what the caps are made of
#   on the CPU (ATen's CPU kernels):      E_loss 7.7 - 8.2 with the thread count (randn_s6_v32000), C_grad 57.2 (randn_s6_v32000)
# The fused path runs on the MI355X, so its bar is the chain it replaces there; the CPU's chain sums in another order and is looser.
EAGER_E_LOSS = 0.597
EAGER_C_GRAD = 50.2
LOSS_CAP = 4 * EAGER_E_LOSS
GRAD_CAP = 4 * EAGER_C_GRAD


def chain(s, t):
    """the reference's three ops (utils/kd_trainer.py:44-47), softmax over the last dimension"""
    return F.kl_div(F.log_softmax(s, dim=-1), F.softmax(t, dim=-1), reduction="batchmean")


def ref64(s, t):
    """the chain in float64 with autograd -> loss64, ds64 (upstream gradient 1), lse_s, lse_t, p_s, p_t (all float64, on s's device)"""
    s64, t64 = s.detach().double().requires_grad_(True), t.detach().double()
    loss = chain(s64, t64)
    (ds,) = torch.autograd.grad(loss, s64)
    s64 = s64.detach()
    lse_s, lse_t = torch.logsumexp(s64, dim=-1), torch.logsumexp(t64, dim=-1)
    return loss.detach(), ds, lse_s, lse_t, torch.exp(s64 - lse_s.unsqueeze(-1)), torch.exp(t64 - lse_t.unsqueeze(-1))


def eager32(s, t):
    """the chain on .float() inputs, which is what CUDA autocast runs -> loss32, ds32 (fp32)"""
    s32, t32 = s.detach().float().requires_grad_(True), t.detach().float()
    loss = chain(s32, t32)
    (ds,) = torch.autograd.grad(loss, s32)
    return loss.detach(), ds


def formula64(s, t):
    """the contract's identity in float64 -> loss, ds, lse_s, lse_t, p_s, p_t as ref64; terms with p_t == 0 contribute 0, also where s
    is -inf (where the chain gives NaN: the one documented deviation)"""
    s64, t64 = s.detach().double(), t.detach().double()
    lse_s, lse_t = torch.logsumexp(s64, dim=-1, keepdim=True), torch.logsumexp(t64, dim=-1, keepdim=True)
    p_s, p_t = torch.exp(s64 - lse_s), torch.exp(t64 - lse_t)
    term = torch.where(p_t == 0, torch.zeros_like(p_t), p_t * (t64 - s64))
    loss = (term.sum(-1, keepdim=True) - lse_t + lse_s).sum() / s.shape[0]
    return loss, (p_s - p_t) / s.shape[0], lse_s.squeeze(-1), lse_t.squeeze(-1), p_s, p_t


def e_loss(x, s, t, ref=None):
    loss64, _, lse_s, lse_t, _, p_t = ref or ref64(s, t)
    d = (t.detach().double() - s.detach().double()).abs()
    n = (lse_s.abs().sum() + lse_t.abs().sum() + torch.where(p_t == 0, torch.zeros_like(p_t), p_t * d).sum()) / s.shape[0]
    return float((x.detach().double().to(loss64.device) - loss64).abs() / n / UNIT)


def c_grad(x, s, t, dtype=torch.float32, g=1.0, ref=None):
    _, ds64, _, _, p_s, p_t = ref or ref64(s, t)
    ds64 = ds64 * g
    num = ((x.detach().double().to(ds64.device) - ds64).abs() - U_OUT[dtype] * ds64.abs() - A_OUT[dtype]).clamp_min(0)
    den = (p_s + p_t) * abs(g) / s.shape[0]
    q = torch.where(num == 0, torch.zeros_like(num), num / den)        # 0 / 0 where both probabilities underflow: no error, no measure
    return float(q.max() / UNIT)


def _randn(shape, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    # bf16-representable values, so that every dtype of the GPU tier but fp16's range limit sees the inputs the caps were measured on
    return (torch.randn(shape, generator=g) * sigma).bfloat16().float(), (torch.randn(shape, generator=g) * sigma).bfloat16().float()


def cases():
    """name -> (s, t): fp32 CPU tensors [rows, V]"""
    out = {}
    for sigma in (1, 3, 6):
        for v in (4099, 32000):
            out[f"randn_s{sigma}_v{v}"] = _randn((4, v), float(sigma), 100 * sigma + v)
    ramp = torch.linspace(-8.0, 8.0, 2049).bfloat16().float()
    out["ramp_v2049"] = (ramp.repeat(2, 1).contiguous(), ramp.flip(0).repeat(2, 1).contiguous())
    out["randn_s30_v33"] = _randn((3, 33), 30.0, 33)
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
    for name, (s, t) in CASES().items():
        s, t = s.to(device), t.to(device)
        ref = ref64(s, t)
        loss, ds = eager32(s, t)
        out[name] = (e_loss(loss, s, t, ref), c_grad(ds, s, t, ref=ref))
    return out
