"""Reference, error measures, case list and caps for the fused RMSNorm (llm_qat_amd.norm).

Given the same rstd the fused forward equals the reference's chain bit for bit (recipe() against chain(), checked on the CPU tier); what can
differ is the last bit of a row's rstd, because the sum of squares runs in another order than ATen's.  So the bars are: recipe(kernel's
rstd) bit for bit, and error against float64 measured beside the eager fp32 chain's own error.  All measures are in units of 2^-24
(fp32's unit roundoff), with u, A the one output rounding and the flush-to-zero allowance of tests/kd_loss_reference.py (U_OUT, A_OUT):

  E_rstd = |rstd - rstd64| / rstd64
  E_y    = (|y - y64| - u |y64| - A)+ / (|w| |n64|)                                   n = x rstd
  C_dx   = (|dx - dx64| - u |dx64| - A)+ / (rstd (|a| + |n| (1/H) sum_c |a n|))        a = g w
  C_dw   = (|dw - dw64| - u |dw64| - A)+ / sum_r |g n|

The denominators are the magnitudes of what is multiplied, subtracted and added up, so the measures are well-conditioned where the results
themselves cancel.  Each cap is 4 x the eager fp32 chain's largest measure over CASES on the MI355X: a factor 2 for the hardware
reciprocal square root against ATen's function, times 2 for another summation order.  They come from the eager chain, never from the kernels.
"""
import torch

from kd_loss_reference import A_OUT, U_OUT, UNIT

EPS = 1e-6

# The eager fp32 chain's largest measures over CASES, as measured by eager_measures():
#   on the MI355X (ROCm's ATen kernels):  E_rstd 2.4606, E_y 3.3795, C_dx 3.6632 (all randn_s0.01_h33), C_dw 3.5144 (randn_s1_h4099)
#                                                                                                 <- what the caps are made of
#   on the CPU (ATen's CPU kernels):      E_rstd 2.5256, C_dx 4.2116 (randn_s1_1030x64), E_y 4.1217, C_dw 3.7605 (randn_s0.01_h4096)
# The fused path runs on the MI355X, so its bar is the chain it replaces there.  (The fused path itself, fp32: 2.17, 3.87, 3.82, 3.52.)
EAGER_E_RSTD = 2.47
EAGER_E_Y = 3.38
EAGER_C_DX = 3.67
EAGER_C_DW = 3.52
RSTD_CAP = 4 * EAGER_E_RSTD
Y_CAP = 4 * EAGER_E_Y
DX_CAP = 4 * EAGER_C_DX
DW_CAP = 4 * EAGER_C_DW


def chain_rstd(x, eps=EPS):
    """the chain's rsqrt(variance + eps), fp32 [rows, 1]"""
    return torch.rsqrt(x.to(torch.float32).pow(2).mean(-1, keepdim=True) + eps)


def chain(x, w, eps=EPS):
    """the reference's lines (models/modeling_llama_quant.py:121-129)"""
    variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = x * torch.rsqrt(variance + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        h = h.to(w.dtype)
    return w * h


def recipe(x, w, rstd):
    """the contract's forward in torch ops, from a given fp32 rstd ([rows] or [..., 1]): one rounding per line"""
    n = x.to(torch.float32) * rstd.reshape(x.shape[:-1] + (1,))
    if w.dtype == torch.float32:
        return w * n
    return (w.to(torch.float32) * n.to(w.dtype).to(torch.float32)).to(w.dtype)


def formula64(x, w, g, eps=EPS):
    """the contract's backward in float64, written out -> dx, dw"""
    x, w, g = x.double(), w.double(), g.double()
    h = x.shape[-1]
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    n, a = x * rstd, g * w
    s = (a * n).sum(-1, keepdim=True) / h
    return rstd * (a - n * s), (g * n).reshape(-1, h).sum(0)


def ref64(x, w, g, eps=EPS):
    """float64 autograd of the unrounded formula -> y64, rstd64 [rows, 1], dx64, dw64, n64, a64 (on x's device)"""
    x64 = x.detach().double().requires_grad_(True)
    w64 = w.detach().double().requires_grad_(True)
    rstd = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    y = w64 * (x64 * rstd)
    dx, dw = torch.autograd.grad(y, (x64, w64), g.detach().double())
    rstd = rstd.detach()
    return y.detach(), rstd, dx, dw, x64.detach() * rstd, g.detach().double() * w64.detach()


def _ratio(num, den):
    return torch.where(num == 0, torch.zeros_like(num), num / den)     # 0 / 0 where a product underflows: no error, no measure


def _excess(got, want, dtype):
    want = want.to(got.device) if want.device != got.device else want
    u, a = (0.0, A_OUT[torch.float32]) if dtype is torch.float64 else (U_OUT[dtype], A_OUT[dtype])
    return ((got.detach().double() - want).abs() - u * want.abs() - a).clamp_min(0)


def e_rstd(rstd, ref):
    r64 = ref[1].reshape(-1)
    return float(((rstd.detach().double().reshape(-1) - r64).abs() / r64).max() / UNIT)


def e_y(y, w, ref):
    return float(_ratio(_excess(y, ref[0], y.dtype), w.detach().double().abs() * ref[4].abs()).max() / UNIT)


def c_dx(dx, ref):
    _, rstd, dx64, _, n, a = ref
    den = rstd * (a.abs() + n.abs() * (a * n).abs().sum(-1, keepdim=True) / n.shape[-1])
    return float(_ratio(_excess(dx, dx64, dx.dtype), den).max() / UNIT)


def c_dw(dw, g, ref):
    den = (g.detach().double() * ref[4]).abs().reshape(-1, ref[4].shape[-1]).sum(0)
    return float(_ratio(_excess(dw, ref[3], dw.dtype), den).max() / UNIT)


def _case(rows, h, sigma, seed):
    gen = torch.Generator().manual_seed(seed)
    # bf16-representable values, so that every dtype of the GPU tier but fp16's range limits sees the inputs the caps were measured on
    x = (torch.randn((rows, h), generator=gen) * sigma).bfloat16().float()
    x[:, 3 % h] = (x[:, 3 % h] * 20).bfloat16().float()            # one column that carries most of a row's sum of squares
    w = (1 + 0.1 * torch.randn(h, generator=gen)).bfloat16().float()
    g = torch.randn((rows, h), generator=gen).bfloat16().float()
    return x, w, g


def cases():
    """name -> (x, w, g): fp32 [rows, H] x and g, [H] w, on the CPU"""
    out = {}
    for sigma in (0.01, 1.0, 30.0):
        for h in (33, 256, 4096, 4099):
            out[f"randn_s{sigma:g}_h{h}"] = _case(8, h, sigma, int(100 * sigma) + h)
    out["randn_s1_64x515"] = _case(64, 515, 1.0, 515)
    out["randn_s1_1030x64"] = _case(1030, 64, 1.0, 1030)
    return out


_CASES = None


def CASES():
    """the case list, built once and shared; callers leave the tensors unchanged"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def eager32(x, w, g, eps=EPS):
    """the chain and its autograd gradients on fp32 tensors -> y, rstd, dx, dw"""
    xr, wr = x.detach().float().requires_grad_(True), w.detach().float().requires_grad_(True)
    y = chain(xr, wr, eps)
    dx, dw = torch.autograd.grad(y, (xr, wr), g.float())
    return y.detach(), chain_rstd(x.float(), eps), dx, dw


def eager_measures(device="cpu"):
    """name -> (E_rstd, E_y, C_dx, C_dw) of the eager fp32 chain on `device`: what the caps are made of"""
    out = {}
    for name, (x, w, g) in CASES().items():
        x, w, g = x.to(device), w.to(device), g.to(device)
        ref = ref64(x, w, g)
        y, rstd, dx, dw = eager32(x, w, g)
        out[name] = (e_rstd(rstd, ref), e_y(y, w, ref), c_dx(dx, ref), c_dw(dw, g, ref))
    return out
