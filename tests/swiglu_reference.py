"""Reference, error measures, case list and caps for the fused SwiGLU (llm_qat_amd.mlp).

The op has no reduction, so its bar is the eager chain's bits: recipe_fwd / recipe_bwd restate the contract of
include/llmqat_fakequant_act.h in torch fp32 ops, chain() is F.silu(g) * u with autograd.  Where bits cannot be compared (ATen's CPU fp16
silu_backward and its vectorised fp32 exp take other routes) the bar is the error against float64, measured against the condition of each
expression and not against its result: dg's factor sig (1 + g (1 - sig)) crosses zero near g = -1.28, where a relative error means
nothing.  All measures are in units of 2^-24 (fp32's unit roundoff), with u, A the one output rounding and the flush-to-zero allowance of
tests/kd_loss_reference.py (U_OUT, A_OUT):

  C_y  = (|y  - y64|  - u |y64|  - A)+ / (|g| sig |u|)
  C_du = (|du - du64| - u |du64| - A)+ / (|dy| |g| sig)
  C_dg = (|dg - dg64| - u |dg64| - A)+ / (|dy u| (sig + |g| sig (1 - sig)))

A 16-bit chain rounds twice on the way to y, du and dg (silu's output, mul's gradient): the measures allow for the inner rounding as they
do for the outer one (_measure says how).  That allowance is a deliberate departure from the formulas above, which have one rounding: without it
the 16-bit chain itself measures in the thousands.  For fp32 the measures are the formulas as they stand.  The caps are 2 x the eager fp32 chain's largest measure over CASES:
they come from the chain, never from the kernels.
"""
import torch
import torch.nn.functional as F

from kd_loss_reference import A_OUT, U_OUT, UNIT

# The eager fp32 chain's largest measures over CASES, as measured by eager_measures():
#   on the CPU (ATen's CPU kernels):      C_y 3.0511 (ramp_16), C_dg 17.4656 (randn_s30), C_du 3.0272 (randn_s1)
#   on the MI355X (ROCm's ATen kernels):  C_y 3.0511 (ramp_16), C_dg 17.4655 (randn_s30), C_du 3.0272 (randn_s1): the same worst cases and values
#                                         (tests/test_gpu_swiglu.py holds the chain within the caps' half there)
EAGER_C_Y = 3.06
EAGER_C_DG = 17.47
EAGER_C_DU = 3.03
Y_CAP = 2 * EAGER_C_Y
DU_CAP = 2 * EAGER_C_DU
DG_CAP = 2 * EAGER_C_DG


def chain(g, u, dy):
    """the eager chain (models/modeling_llama_quant.py:235 with act_fn = SiLU) and its autograd -> y, dg, du"""
    gr, ur = g.detach().clone().requires_grad_(True), u.detach().clone().requires_grad_(True)
    y = F.silu(gr) * ur
    dg, du = torch.autograd.grad(y, (gr, ur), dy)
    return y.detach(), dg, du


def _rb(t, dtype):
    return t.to(dtype).float()


def recipe_fwd(g, u):
    """the contract's forward in torch fp32 ops, one rounding per line"""
    dt = g.dtype
    gf, uf = g.float(), u.float()
    a = gf / (1.0 + torch.exp(-gf))
    return (_rb(a, dt) * uf).to(dt)


def recipe_bwd(dy, g, u, fma=True):
    """the contract's backward in torch fp32 ops -> dg, du.  fma: 1 + g (1 - sig) rounded once (through float64, where the product of two
    fp32 values is exact and the sum is rounded to 53 bits before it is rounded to 24, which differs from an fma only on a double-rounding
    tie), as ATen's device code; else a rounded product and a rounded sum"""
    dt = g.dtype
    df, gf, uf = dy.float(), g.float(), u.float()
    den = 1.0 + torch.exp(-gf)
    sig = 1.0 / den
    a = _rb(gf / den, dt)
    ds = _rb(df * uf, dt)
    du = (df * a).to(dt)
    t = (1.0 + gf.double() * (1.0 - sig).double()).float() if fma else 1.0 + gf * (1.0 - sig)
    return ((ds * sig) * t).to(dt), du


def ref64(g, u, dy):
    """float64 autograd of the unrounded function -> y64, dg64, du64, sig64 (on g's device)"""
    g64, u64 = g.detach().double().requires_grad_(True), u.detach().double().requires_grad_(True)
    y = F.silu(g64) * u64
    dg, du = torch.autograd.grad(y, (g64, u64), dy.detach().double())
    return y.detach(), dg, du, torch.sigmoid(g64.detach())


def _measure(got, want, cond, dtype, inner, scale):
    """(|got - want| - u |want| - A - inner allowance)+ / cond, largest, in units of 2^-24.  The inner allowance is for a 16-bit chain's
    first rounding (none for fp32): an intermediate of magnitude `inner` is rounded to the dtype, an error of at most u inner + A, and
    reaches the result multiplied by `scale`; the result's own rounding sees it once more (1 + u)"""
    u, a = (0.0, A_OUT[torch.float32]) if dtype is torch.float64 else (U_OUT[dtype], A_OUT[dtype])
    want = want.to(got.device)
    slack = u * want.abs() + a
    if u:
        slack = slack + (u * inner + a) * scale * (1 + u)
    num = ((got.detach().double() - want).abs() - slack).clamp_min(0)
    return float(torch.where(num == 0, torch.zeros_like(num), num / cond).max() / UNIT)


def measures(y, dg, du, g, u, dy, ref=None):
    """-> (C_y, C_dg, C_du) of results in the dtype of y.  The inner roundings: silu's output a (times |u| in y, times |dy| in du) and
    mul's gradient dy u (times silu's derivative in dg)"""
    y64, dg64, du64, sig = ref or ref64(g, u, dy)
    g64, u64, d64 = g.detach().double(), u.detach().double(), dy.detach().double()
    a = g64.abs() * sig
    c_y = _measure(y, y64, a * u64.abs(), y.dtype, a, u64.abs())
    c_du = _measure(du, du64, d64.abs() * a, du.dtype, a, d64.abs())
    cond = (d64 * u64).abs() * (sig + g64.abs() * sig * (1 - sig))
    c_dg = _measure(dg, dg64, cond, dg.dtype, (d64 * u64).abs(), (sig * (1 + g64 * (1 - sig))).abs())
    return c_y, c_dg, c_du


def _case(shape, sigma, seed):
    gen = torch.Generator().manual_seed(seed)
    # bf16-representable values, so that every dtype of the GPU tier but fp16's range limits sees the inputs the caps were measured on
    g = (torch.randn(shape, generator=gen) * sigma).bfloat16().float()
    u = torch.randn(shape, generator=gen).bfloat16().float()
    dy = torch.randn(shape, generator=gen).bfloat16().float()
    return g, u, dy


def cases():
    """name -> (g, u, dy): fp32 tensors on the CPU.  sigma = 3 reaches both tails of the sigmoid and the zero of its derivative's factor;
    30 the range where exp(-g) overflows; the ramp holds every bf16 value of [-16, 16] around that zero"""
    out = {f"randn_s{sigma:g}": _case((64, 515), sigma, 27 + int(10 * sigma)) for sigma in (0.1, 1.0, 3.0, 30.0)}
    ramp = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    ramp = ramp[ramp.abs() <= 16].reshape(1, -1)
    gen = torch.Generator().manual_seed(5)
    out["ramp_16"] = (ramp, torch.randn(ramp.shape, generator=gen).bfloat16().float(), torch.randn(ramp.shape, generator=gen).bfloat16().float())
    return out


_CASES = None


def CASES():
    """the case list, built once and shared; callers leave the tensors unchanged"""
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES


def eager_measures(device="cpu"):
    """name -> (C_y, C_dg, C_du) of the eager fp32 chain on `device`: what the caps are made of"""
    out = {}
    for name, (g, u, dy) in CASES().items():
        g, u, dy = g.to(device), u.to(device), dy.to(device)
        y, dg, du = chain(g, u, dy)
        out[name] = measures(y, dg, du, g, u, dy)
    return out
