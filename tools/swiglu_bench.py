#!/usr/bin/env python
"""The fused SwiGLU (llm_qat_amd.mlp.swiglu) beside the eager chain it replaces, on MI355X.

  shapes   bf16 [2048, 11008], [8192, 11008] and [2048, 13824] gate, up and dy
  fused    swiglu forward (one kernel), backward (one kernel), and their sum
  eager    F.silu(gate) * up under torch.autocast("cuda", bf16), then .backward(dy)
  timing   HIP events around each phase, the inputs rotated so that no call finds its tensors in the 256 MiB Infinity Cache; median and
           spread (min, max) over --iters calls after --warmup
  rates    event_time_fraction_of_pin_rate: the fused path's bytes over the EVENT time of a phase against the 8 TB/s pin rate, counting
           6 B/element forward (gate and up read, y written) and 10 B/element backward (dy, gate and up read, dgate and dup written).
           The event time holds the host's enqueue gaps, so this is the rate a caller sees, not a kernel's: the kernels' own rates come
           from a kernel trace (profiles/swiglu_kernel_times.txt)
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/swiglu_bench.py [--out profiles/swiglu_bench.json] [--iters 30] [--warmup 5] [--fused-only]

--fused-only leaves the eager chain out: for A/B runs of kernel variants (build.py -DSWIGLU_NT_STORE=0 --out=..., then
LLMQAT_AMD_LIB=... python tools/swiglu_bench.py --fused-only --out ...) and for kernel traces.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_qat_amd.mlp import swiglu  # noqa: E402

PIN_RATE = 8.0e12   # bytes per second


def eager_swiglu(g, u):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return F.silu(g) * u


def time_path(fn, sets, iters, warmup):
    """-> per-call milliseconds of the forward and of the backward"""
    fwd, bwd = [], []
    for i in range(warmup + iters):
        g, u, dy = sets[i % len(sets)]
        g.grad = u.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        y = fn(g, u)
        e[1].record()
        y.backward(dy)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    return fwd, bwd


def peak(fn, g, u, dy):
    g.grad = u.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn(g, u)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    y.backward(dy)
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    g.grad = u.grad = None
    return fwd_peak, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swiglu_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swiglu_bench needs the GPU: a timing taken elsewhere says nothing")
    from llm_qat_amd import _lib
    _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "shapes": {}}
    for rows, cols in ((2048, 11008), (8192, 11008), (2048, 13824)):
        n = rows * cols
        nsets = max(2, -(-(600 << 20) // (6 * n)))       # gate, up and dy of every set: more than twice the 256 MiB Infinity Cache in rotation
        gen = torch.Generator(device="cuda").manual_seed(rows + cols)
        sets = []
        for _ in range(nsets):
            g = (torch.randn((rows, cols), device="cuda", generator=gen) * 3).bfloat16().requires_grad_(True)
            u = torch.randn((rows, cols), device="cuda", dtype=torch.bfloat16, generator=gen).requires_grad_(True)
            sets.append((g, u, torch.randn((rows, cols), device="cuda", dtype=torch.bfloat16, generator=gen)))
        entry = {"elements": n, "input_sets": nsets}
        for name, fn in (("fused", swiglu),) + (() if args.fused_only else (("eager", eager_swiglu),)):
            fwd, bwd = time_path(fn, sets, args.iters, args.warmup)
            both = [a + b for a, b in zip(fwd, bwd)]
            pf, pb = peak(fn, *sets[0])
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "forward_peak_bytes_over_inputs": pf, "peak_bytes_over_inputs": pb}
        f = entry["fused"]
        f["forward"]["event_time_fraction_of_pin_rate"] = round(6 * n / (f["forward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        f["backward"]["event_time_fraction_of_pin_rate"] = round(10 * n / (f["backward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        if not args.fused_only:
            fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
            entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
            entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]       # the gate: the fused path's slowest call beats the eager chain's fastest
        result["shapes"][f"{rows}x{cols}"] = entry
        del sets
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    if not args.fused_only and not all(e["faster_beyond_spread"] for e in result["shapes"].values()):
        raise SystemExit("gate missed: at some shape the fused forward plus backward's slowest call is not faster than the eager chain's fastest")


if __name__ == "__main__":
    main()
