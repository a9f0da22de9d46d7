#!/usr/bin/env python3
"""Recorded results of the REAL reference for tests/test_oracle_vs_live_reference.py -> tests/golden/live_reference.json.

Runs the reference's own `SymQuantizer` / `AsymQuantizer` / `QuantizeLinear` (models/utils_quant.py) on the inputs the tests draw
(the case generators of the test modules, same seeds) and records digests of the inputs and of what the reference computed:

    fresh        forward value + STE gradient, 3 dtypes x 150 trials
    autocast     SymQuantizer.apply under CUDA autocast's cast policy (tests/autocast_policy.py), 2 dtypes x both scalar policies x 75
    lowbit       the weight QuantizeLinear's 1-/2-bit branches hand to F.linear, 3 dtypes x 50
    degenerate   results (float32 bit patterns) or exception type names on tensors without elements / with one element

    PYTHONDONTWRITEBYTECODE=1 LLMQAT_REFERENCE=<checkout of the reference> python tests/golden/make_golden_live_reference.py

Runs only where the reference is present; the .json holds digests and small results, nothing of the reference's text.
"""
import json
import os
import sys
import warnings

sys.dont_write_bytecode = True
REF = os.environ.get("LLMQAT_REFERENCE")
if not REF or not os.path.isfile(os.path.join(REF, "models", "utils_quant.py")):
    sys.exit("set LLMQAT_REFERENCE to a checkout of the reference (models/utils_quant.py)")
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_oracle_vs_live_reference as T  # noqa: E402
from autocast_policy import cuda_autocast_policy  # noqa: E402

sys.path.insert(0, REF)
import models.utils_quant as R  # noqa: E402

sys.path.remove(REF)


def fresh(dtype):
    out = []
    for trial, x, kind, bits, layerwise, lo, hi, g in T.fresh_cases(dtype):
        quant = R.SymQuantizer if kind == "sym" else R.AsymQuantizer
        xr = x.clone().requires_grad_(True)
        with np.errstate(all="ignore"):
            y = quant.apply(xr, torch.tensor([lo, hi]), bits, layerwise)
            y.backward(g)
        out.append({"x": T.digest(T.to_np(x), dtype), "g": T.digest(T.to_np(g), dtype),
                    "y": T.digest(T.to_np(y), dtype), "gx": T.digest(T.to_np(xr.grad), dtype)})
    return out


def autocast(dtype, device_scalars):
    out = []
    for trial, x, bits, lo, hi, g in T.autocast_cases(dtype, device_scalars):
        xr = x.clone().requires_grad_(True)
        with cuda_autocast_policy(T.TD[dtype], device_scalars), np.errstate(all="ignore"):
            y = R.SymQuantizer.apply(xr, torch.tensor([lo, hi]), bits, False)
        assert y.dtype == torch.float32
        y.backward(g)
        out.append({"x": T.digest(T.to_np(x), dtype), "g": T.digest(g.numpy(), "fp32"),
                    "y": T.digest(y.detach().numpy(), "fp32"), "gx": T.digest(T.to_np(xr.grad), dtype)})
    return out


def lowbit(dtype):
    import torch.nn.functional as F
    seen, real = {}, F.linear

    def spy(inp, weight, bias=None):
        seen["w"] = weight.detach().clone()
        return real(inp, weight, bias)

    out = []
    R.nn.functional.linear = spy
    try:
        for trial, out_f, in_f, w_bits, layerwise, weight in T.lowbit_cases(dtype):
            lin = R.QuantizeLinear(in_f, out_f, w_bits=w_bits, a_bits=32, weight_layerwise=layerwise).to(T.TD[dtype])
            with torch.no_grad():
                lin.weight.copy_(weight)
                lin(torch.zeros(2, in_f, dtype=T.TD[dtype]))
            out.append({"w": T.digest(T.to_np(lin.weight), dtype), "linear_weight": T.digest(T.to_np(seen["w"]), dtype)})
    finally:
        R.nn.functional.linear = real
    return out


def degenerate():
    return {f"{name} {shape} layerwise={layerwise}": T.run_degenerate(q, shape, layerwise)
            for shape in T.DEGENERATE_SHAPES for layerwise in (False, True)
            for name, q in (("SymQuantizer", R.SymQuantizer), ("AsymQuantizer", R.AsymQuantizer))}


if __name__ == "__main__":
    warnings.simplefilter("ignore")
    rec = {"meta": {"what": "digests of the reference's results (tests/test_oracle_vs_live_reference.py: digest)",
                    "torch": torch.__version__, "numpy": np.__version__},
           "fresh": {d: fresh(d) for d in ("bf16", "fp16", "fp32")},
           "autocast": {f"{d}/{int(s)}": autocast(d, s) for d in ("bf16", "fp16") for s in (False, True)},
           "lowbit": {d: lowbit(d) for d in ("bf16", "fp16", "fp32")},
           "degenerate": degenerate()}
    path = os.path.join(HERE, "live_reference.json")
    with open(path, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
