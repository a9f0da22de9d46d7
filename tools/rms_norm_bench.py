#!/usr/bin/env python
"""The fused RMSNorm (llm_qat_amd.norm.rms_norm) beside the eager lines it replaces, on MI355X.

  shapes   bf16 [2048, 4096], [8192, 4096] and [2048, 5120] hidden states, a bf16 weight
  fused    rms_norm forward (one kernel), backward (the rows, then the sum over the parts), and their sum
  eager    the reference's lines (LlamaRMSNorm.forward) under torch.autocast("cuda", bf16), then .backward(g)
  timing   HIP events around each phase, the inputs rotated so that no call finds its tensors in the 256 MiB Infinity Cache; median and
           spread (min, max) over --iters calls after --warmup
  rates    event_time_fraction_of_pin_rate: the fused path's bytes over the EVENT time of a phase against the 8 TB/s pin rate, counting
           4 B/element forward (x read, y written) and 6 B/element backward (g and x read, dx written) plus the partial sums
           (written and read once: 8 B each).  The event time holds the host's enqueue gaps, so this is the rate a caller sees, not a
           kernel's: the kernels' own rates come from a kernel trace (profiles/rms_norm_kernel_times.txt)
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/rms_norm_bench.py [--out profiles/rms_norm_bench.json] [--iters 30] [--warmup 5] [--fused-only]

--fused-only leaves the eager chain out: for A/B runs of kernel variants (build.py -DRMS_NT_STORE=0 --out=..., then
LLMQAT_AMD_LIB=... python tools/rms_norm_bench.py --fused-only --out ...) and for kernel traces.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_qat_amd.norm import rms_norm  # noqa: E402

PIN_RATE = 8.0e12   # bytes per second
EPS = 1e-6


def eager_norm(x, w):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
        h = x * torch.rsqrt(variance + EPS)
        if w.dtype in (torch.float16, torch.bfloat16):
            h = h.to(w.dtype)
        return w * h


def fused_norm(x, w):
    return rms_norm(x, w, EPS)


def time_path(fn, sets, w, iters, warmup):
    """-> per-call milliseconds of the forward and of the backward"""
    fwd, bwd = [], []
    for i in range(warmup + iters):
        x, g = sets[i % len(sets)]
        x.grad = w.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        y = fn(x, w)
        e[1].record()
        y.backward(g)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    return fwd, bwd


def peak(fn, x, g, w):
    x.grad = w.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn(x, w)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    y.backward(g)
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    x.grad = w.grad = None
    return fwd_peak, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rms_norm_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rms_norm_bench needs the GPU: a timing taken elsewhere says nothing")
    from llm_qat_amd import _lib
    L = _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "shapes": {}}
    for rows, cols in ((2048, 4096), (8192, 4096), (2048, 5120)):
        n = rows * cols
        nsets = max(2, -(-(600 << 20) // (4 * n)))       # x and g of every set: more than twice the 256 MiB Infinity Cache in rotation
        gen = torch.Generator(device="cuda").manual_seed(rows + cols)
        w = (1 + 0.1 * torch.randn(cols, device="cuda", generator=gen)).bfloat16().requires_grad_(True)
        sets = []
        for _ in range(nsets):
            x = torch.randn((rows, cols), device="cuda", dtype=torch.bfloat16, generator=gen).requires_grad_(True)
            sets.append((x, torch.randn((rows, cols), device="cuda", dtype=torch.bfloat16, generator=gen)))
        parts = L.fqn_rms_norm_bwd_parts(rows, cols)
        entry = {"elements": n, "input_sets": nsets, "backward_parts": parts}
        for name, fn in (("fused", fused_norm),) + (() if args.fused_only else (("eager", eager_norm),)):
            fwd, bwd = time_path(fn, sets, w, args.iters, args.warmup)
            both = [a + b for a, b in zip(fwd, bwd)]
            pf, pb = peak(fn, *sets[0], w)
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "forward_peak_bytes_over_inputs": pf, "peak_bytes_over_inputs": pb}
        f = entry["fused"]
        f["forward"]["event_time_fraction_of_pin_rate"] = round(4 * n / (f["forward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        f["backward"]["event_time_fraction_of_pin_rate"] = round((6 * n + 8 * parts * cols) / (f["backward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        if not args.fused_only:
            fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
            entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
            entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]
        result["shapes"][f"{rows}x{cols}"] = entry
        del sets
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
