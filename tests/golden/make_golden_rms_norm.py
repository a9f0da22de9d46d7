#!/usr/bin/env python3
"""Golden vectors of the reference's own LlamaRMSNorm (models/modeling_llama_quant.py:112-129) on CPU tensors -> rms_norm.npz.

    LLMQAT_REFERENCE=<checkout of the reference> python tests/golden/make_golden_rms_norm.py

For the three equal-dtype pairs and two mixed ones (x dtype _ weight dtype) at H = 7, 33 and 256: x, w, eps, g -> y, dx over every row, and
dw over the regular rows (a NaN row would make every dw NaN).  Rows 0 .. REGULAR-1 are randn; then a zero row, a row with a NaN, a row
with an inf and a row with 1e20, whose square overflows fp32 (fp16 has no 1e20: there it is a second inf row).  16-bit values are stored
as bit patterns (uint16).  Only the generator reads the reference; the tests read the .npz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if "LLMQAT_REFERENCE" not in os.environ:
    raise SystemExit("set LLMQAT_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["LLMQAT_REFERENCE"])

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.modeling_llama_quant import LlamaRMSNorm  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f32", "f32"), ("bf16", "f32"), ("f32", "bf16")]
HS = (7, 33, 256)
REGULAR = 2
SPECIAL = ("zero", "nan", "inf", "overflow")


def store(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy()


def main():
    out = {"pairs": np.array(["_".join(p) for p in PAIRS]), "hs": np.array(HS), "regular": np.array(REGULAR), "special": np.array(SPECIAL)}
    for pi, (xd, wd) in enumerate(PAIRS):
        for h in HS:
            gen = torch.Generator().manual_seed(1000 * pi + h)
            eps = 1e-6 if h != 33 else 1e-5
            x = torch.randn((REGULAR + len(SPECIAL), h), generator=gen) * 1.5
            x[REGULAR] = 0.0
            x[REGULAR + 1, h // 2] = float("nan")
            x[REGULAR + 2, h - 1] = float("-inf")
            x[REGULAR + 3, 0] = 1e20
            x = x.to(DT[xd])
            w = (1 + 0.1 * torch.randn(h, generator=gen)).to(DT[wd])
            m = LlamaRMSNorm(h, eps=eps)
            m.weight.data = w.clone()
            xr = x.clone().requires_grad_(True)
            y = m(xr)
            g = torch.randn(y.shape, generator=gen).to(y.dtype)
            (dx,) = torch.autograd.grad(y, xr, g)
            xr = x[:REGULAR].clone().requires_grad_(True)
            (dw,) = torch.autograd.grad(m(xr), m.weight, g[:REGULAR])
            assert y.dtype == DT[wd] and dx.dtype == DT[xd] and dw.dtype == DT[wd]
            k = f"{xd}_{wd}_h{h}_"
            out.update({k + "x": store(x), k + "w": store(w), k + "eps": np.array(eps), k + "g": store(g), k + "y": store(y), k + "dx": store(dx),
                        k + "dw": store(dw)})
    path = os.path.join(HERE, "rms_norm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
