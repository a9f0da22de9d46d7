#!/usr/bin/env python3
"""Generate tests/golden/group.npz: group-wise fake quantization pinned to the reference's own classes.

Group-wise scales are the reference's SymQuantizer / AsymQuantizer (models/utils_quant.py:37-74, :96-149, layerwise=False) applied to the
[rows * C / g, g] view of a tensor:  y = Q(x.reshape(-1, g)).reshape(x.shape).  This script imports the real reference module on CPU, runs
its classes on such views and records inputs + outputs (data only, as the other make_golden*.py do).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_group.py

Cases: Sym / Asym x bf16 / fp16 / fp32 x bits 3 / 4 / 8 x g 32 / 64 / 128 / 256 on [2, 512] tensors whose groups include NaN, +-Inf,
+-0, an all-zero group and a group at the dtype's range ends.  Storage: 16-bit tensors as raw uint16 bit patterns, fp32 as float32;
`manifest` (JSON) lists every case.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("LLMQAT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.utils_quant import AsymQuantizer, SymQuantizer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CLIP = torch.tensor([-2.0, 2.0])
ROWS, COLS = 2, 512


def to_np(t):
    t = t.detach().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype in (torch.bfloat16, torch.float16) else t.numpy()


def make_input(dt, g, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, COLS, generator=gen, dtype=torch.float32) * 0.05
    x = x.to(DT[dt])
    big = torch.finfo(DT[dt]).max
    tiny = torch.finfo(DT[dt]).tiny
    v = x.view(ROWS, COLS // g, g)
    v[0, 0, 3] = float("nan")          # a NaN poisons its own group only
    v[0, 1 % (COLS // g), 5] = float("inf") if COLS // g > 1 else v[0, 0, 5]
    v[0, -1, 7] = -float("inf")
    v[1, 0] = 0.0                       # an all-zero group (with a -0)
    v[1, 0, 1] = -0.0
    if COLS // g > 2:
        v[1, 1, 0] = big                # range ends
        v[1, 1, 1] = -big
        v[1, 2, :] = tiny * torch.arange(g, dtype=torch.float32).to(DT[dt])
    return x


def main():
    arrays, cases = {}, []
    k = 0
    for kind in ("sym", "asym"):
        Q = SymQuantizer if kind == "sym" else AsymQuantizer
        for dt in ("bf16", "fp16", "fp32"):
            for bits in (3, 4, 8):
                for g in (32, 64, 128, 256):
                    x = make_input(dt, g, 1000 + k)
                    y = Q.apply(x.reshape(-1, g), CLIP, bits, False).reshape(x.shape)
                    assert y.dtype == x.dtype
                    name = f"c{k}"
                    arrays[name + "_x"] = to_np(x)
                    arrays[name + "_y"] = to_np(y)
                    cases.append({"name": name, "kind": kind, "dtype": dt, "bits": bits, "group": g, "shape": [ROWS, COLS]})
                    k += 1
    arrays["manifest"] = np.array(json.dumps({"cases": cases, "semantics": "cpu_eager", "clip": [-2.0, 2.0]}))
    out = os.path.join(HERE, "group.npz")
    np.savez_compressed(out, **arrays)
    print(out, len(cases), "cases", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
