"""Case list, seeded inputs and cap for the fused prefill attention (llm_qat_amd.attention.prefill_attention).  The
float64 chain, the error measure C_out and the masks are attn_decode_reference's; the cap is 4 x the composed path's (matmul,
attn_softmax, matmul) largest C_out over cases() on the MI355X, by tools/attn_prefill_bench.py --measure."""
import functools
import itertools

import torch

from attn_decode_reference import U, c_out, inv_of, mask_of, ref64  # noqa: F401
from llm_qat_amd.ops import PREFILL_KT as KT, PREFILL_QT as QT

B, H = 2, 3
DIMS = list(itertools.product((64, 128), (torch.bfloat16, torch.float16), ("none", "ds", "f32", "causal")))
TS = (1, 17, QT - 1, QT, QT + 1, 2 * QT + 3)
POOL = 2 * QT + 3 + KT

# Largest C_out over DIMS x cases() (476 cases) on the MI355X, by tools/attn_prefill_bench.py --measure:
#   the composed path:  1.79659 (D 128, fp16, masked, T 128, S 159)      <- what the cap is made of: 4 x 1.7965 = 7.186
#   the fused kernel:   1.65678 (D 64, bf16, masked, T 17, S 17)         beside it, never part of the cap
COMPOSED_C_OUT = 1.7965
CAP = 4 * COMPOSED_C_OUT


def cases(kind):
    """(T, S): every query-tile boundary against every key-tile boundary, and one S < T where no causal rule forbids it"""
    out = [(T, S) for T in TS for S in (T, T + 1, T + KT - 1, T + KT, 2 * KT + 1) if kind != "causal" or T <= S]
    return out + ([] if kind == "causal" else [(QT + 1, KT + 1)])


@functools.lru_cache(maxsize=None)
def _pool(D, dtype, device, seed):
    g = torch.Generator().manual_seed(seed * 100003 + D)
    q, k = (torch.randint(-8, 9, (B, H, POOL, D), generator=g).float() / 4 for _ in range(2))
    return q.to(dtype).to(device), k.to(dtype).to(device), torch.randn((B, H, POOL, D), generator=g).to(dtype).to(device)


def inputs(T, S, D, dtype, device, seed=0, signed_v=False):
    """attn_decode_reference.inputs for any T, and row 1 of EVERY query tile zero: a uniform average that a dropped or doubled key tile moves"""
    q, k, v = (t[:, :, :n].clone() for t, n in zip(_pool(D, dtype, device, seed), (T, S, S)))
    v = v if signed_v else v.abs() + 0.25
    q[:, :, 0] = 2.0
    q[:, :, 1::QT] = 0.0
    for i, (key, zeros) in reversed(list(enumerate(((0, 0), (S - 1, 3), (S // 2, 6))))):
        k[:, :, key] = 2.0
        k[:, :, key, :zeros] = 0.0
        v[:, :, key] = 4.0 * 2 ** i
    return q, k, v


def case_args(kind, T, S, D, dtype, device):
    """-> (q, k, v, the mask of the call, causal of the call, the mask of the float64 reference)"""
    q, k, v = inputs(T, S, D, dtype, device)
    if kind == "causal":
        return q, k, v, None, True, mask_of("ds", T, S, dtype, device)
    mask = mask_of(kind, T, S, dtype, device, batch=B if S % 2 else 1, pad=S // 4)      # both batch strides, left padding
    return q, k, v, mask, False, mask
