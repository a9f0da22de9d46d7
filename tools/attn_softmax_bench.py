#!/usr/bin/env python
"""The fused attention softmax (llm_qat_amd.attention) beside the eager chain it replaces, on MI355X.

  shapes   bf16 scores of [1, 32, 2048, 2048] (7B), [1, 40, 2048, 2048] (13B) and [4, 32, 1024, 1024] with the fp32 causal mask
           [B, 1, T, S] (what bf16 autocast over fp32 weights runs: the sum promotes), and the first shape with a bf16 mask (..._mask_bf16)
  eager    the reference's four lines under torch.autocast("cuda", bfloat16): the division, the sum with the mask, the clamp, the fp32
           softmax and its cast; then autograd's backward
  fused    attention.attn_softmax on the same arguments: one kernel forward, one backward
  timing   HIP events around each phase, the two paths alternating call by call, the inputs rotated (two sets of scores and gradients,
           each set larger than the 256 MiB Infinity Cache); median and spread (min, max) over --iters calls after --warmup
  rates    event_time_bytes_per_s: the fused path's bytes (forward: scores read, y written; backward: scores and g read, dx written; the
           mask's bytes, B T S of them once, are left out) over the EVENT time of a phase: the rate a caller sees, not a kernel's
  yardstick  fqa_swiglu_fwd (ops.swiglu_forward) on [rows, 4096] bf16 at the forward's byte volume, timed the same way in the same process
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/attn_softmax_bench.py [--out profiles/attn_softmax_bench.json] [--iters 30] [--warmup 5] [--fused-only]

--fused-only leaves the eager chain out: for A/B runs of kernel variants (build.py -DATTN_NT_STORE=0 --out=..., then
LLMQAT_AMD_LIB=... python tools/attn_softmax_bench.py --fused-only --out ...) and for kernel traces.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_qat_amd import attention, ops  # noqa: E402

HEAD_DIM = 128
CASES = ((1, 32, 2048, 2048, torch.float32), (1, 40, 2048, 2048, torch.float32), (4, 32, 1024, 1024, torch.float32), (1, 32, 2048, 2048, torch.bfloat16))


def eager_chain(scores, mask, head_dim):
    attn = scores / math.sqrt(head_dim)
    attn = attn + mask
    attn = torch.max(attn, torch.tensor(torch.finfo(attn.dtype).min))
    return torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32).to(scores.dtype)


def time_paths(paths, sets, mask, iters, warmup):
    """-> {name: (forward ms, backward ms)}, the paths alternating call by call"""
    out = {name: ([], []) for name, _ in paths}
    for i in range(warmup + iters):
        x, g = sets[i % len(sets)]
        for name, fn in paths:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                e[0].record()
                y = fn(x, mask, HEAD_DIM)
                e[1].record()
            y.backward(g)
            e[2].record()
            torch.cuda.synchronize()
            x.grad = None
            del y
            if i >= warmup:
                out[name][0].append(e[0].elapsed_time(e[1]))
                out[name][1].append(e[1].elapsed_time(e[2]))
    return out


def time_calls(fn, sets, iters, warmup):
    ms = []
    for i in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn(*sets[i % len(sets)])
        e[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e[0].elapsed_time(e[1]))
    return ms


def peak(fn, x, g, mask):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fn(x, mask, HEAD_DIM)
    y.backward(g)
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    x.grad = None
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_softmax_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_softmax_bench needs the GPU: a timing taken elsewhere says nothing")
    from llm_qat_amd import _lib
    _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "head_dim": HEAD_DIM, "shapes": {}}
    for B, H, T, S, mdt in CASES:
        n = B * H * T * S
        fwd_bytes, bwd_bytes = 4 * n, 6 * n
        gen = torch.Generator(device="cuda").manual_seed(B + H)
        sets = [((torch.randn((B, H, T, S), device="cuda", dtype=torch.bfloat16, generator=gen) * 8).requires_grad_(True),
                 torch.randn((B, H, T, S), device="cuda", dtype=torch.bfloat16, generator=gen)) for _ in range(2)]
        mask = torch.full((T, S), torch.finfo(mdt).min, device="cuda", dtype=mdt).triu(1 + S - T).expand(B, 1, T, S).contiguous()
        paths = (("fused", attention.attn_softmax),) + (() if args.fused_only else (("eager", eager_chain),))
        entry = {"elements": n, "mask_dtype": str(mdt).replace("torch.", ""), "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes, "mask_bytes": mask.numel() * mask.element_size()}
        for name, (fwd, bwd) in time_paths(paths, sets, mask, args.iters, args.warmup).items():
            both = [a + b for a, b in zip(fwd, bwd)]
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "peak_bytes_over_inputs": peak(dict(paths)[name], *sets[0], mask)}
        f = entry["fused"]
        for phase, nb in (("forward", fwd_bytes), ("backward", bwd_bytes)):
            f[phase]["event_time_bytes_per_s"] = round(nb / (f[phase]["median_ms"] * 1e-3) / 1e12, 3) * 1e12
        if not args.fused_only:
            fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
            entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
            entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]       # the gate: the fused path's slowest call beats the eager chain's fastest
        del sets
        torch.cuda.empty_cache()
        rows = round(fwd_bytes / 6 / 4096)                # the yardstick: swiglu's forward at the forward's byte volume
        ysets = [(torch.randn((rows, 4096), device="cuda", dtype=torch.bfloat16, generator=gen), torch.randn((rows, 4096), device="cuda", dtype=torch.bfloat16, generator=gen))
                 for _ in range(2)]
        ms = time_calls(ops.swiglu_forward, ysets, args.iters, args.warmup)
        entry["yardstick_swiglu_forward"] = dict(summary(ms), shape=[rows, 4096], bytes=6 * rows * 4096,
                                                 event_time_bytes_per_s=round(6 * rows * 4096 / (statistics.median(ms) * 1e-3) / 1e12, 3) * 1e12)
        del ysets
        result["shapes"][f"{B}x{H}x{T}x{S}" + ("_mask_bf16" if mdt is torch.bfloat16 else "")] = entry
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
