#!/usr/bin/env python3
"""Golden vectors of the reference's own LlamaMLP.forward (models/modeling_llama_quant.py:234-235, act_fn = ACT2FN["silu"]) on CPU tensors
-> swiglu.npz.

    LLMQAT_REFERENCE=<checkout of the reference> python tests/golden/make_golden_swiglu.py

The reference's forward runs over stand-in projections: gate_proj and up_proj hand back the given gate and up, down_proj is the identity,
so its result is act_fn(gate) * up and autograd's gradients are the chain's.  For bf16, fp16 and fp32 at 7, 33 and 256 columns: gate
(randn, sigma 3), up, dy -> y, dgate, dup over ROWS rows; and per dtype one special row: every pair of
+inf, -inf, NaN, -200, -104, -88, 88, 200, 0, -0 in gate with 0, 1, -1, inf in up.  16-bit values are stored as bit patterns (uint16).
Only the generator reads the reference; the tests read the .npz."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if "LLMQAT_REFERENCE" not in os.environ:
    raise SystemExit("set LLMQAT_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["LLMQAT_REFERENCE"])

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.modeling_llama_quant import ACT2FN, LlamaMLP  # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
COLS = (7, 33, 256)
ROWS = 1
GATES = (float("inf"), float("-inf"), float("nan"), -200.0, -104.0, -88.0, 88.0, 200.0, 0.0, -0.0)
UPS = (0.0, 1.0, -1.0, float("inf"))


class Given(torch.nn.Module):
    """a projection that hands back a given tensor"""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        return self.t


def store(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.element_size() == 2 else t.numpy()


def reference(gate, up, dy):
    mlp = LlamaMLP.__new__(LlamaMLP)
    torch.nn.Module.__init__(mlp)
    g, u = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    mlp.gate_proj, mlp.up_proj, mlp.down_proj, mlp.act_fn = Given(g), Given(u), torch.nn.Identity(), ACT2FN["silu"]
    y = mlp(None)
    dg, du = torch.autograd.grad(y, (g, u), dy)
    assert y.dtype == dg.dtype == du.dtype == gate.dtype
    return y, dg, du


def main():
    out = {"dtypes": np.array(list(DT)), "cols": np.array(COLS), "gates": np.array(GATES, dtype=np.float32), "ups": np.array(UPS, dtype=np.float32)}
    for di, (name, dt) in enumerate(DT.items()):
        for c in COLS:
            gen = torch.Generator().manual_seed(100 * di + c)
            gate = (torch.randn((ROWS, c), generator=gen) * 3).to(dt)
            up, dy = torch.randn((ROWS, c), generator=gen).to(dt), torch.randn((ROWS, c), generator=gen).to(dt)
            y, dg, du = reference(gate, up, dy)
            k = f"{name}_c{c}_"
            out.update({k + "g": store(gate), k + "u": store(up), k + "dy": store(dy), k + "y": store(y), k + "dg": store(dg), k + "du": store(du)})
        gate = torch.tensor(GATES).repeat_interleave(len(UPS)).reshape(1, -1).to(dt)
        up = torch.tensor(UPS).repeat(len(GATES)).reshape(1, -1).to(dt)
        dy = torch.ones_like(up)
        y, dg, du = reference(gate, up, dy)
        k = f"{name}_special_"
        out.update({k + "g": store(gate), k + "u": store(up), k + "dy": store(dy), k + "y": store(y), k + "dg": store(dg), k + "du": store(du)})
    path = os.path.join(HERE, "swiglu.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
