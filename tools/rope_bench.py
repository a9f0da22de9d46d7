#!/usr/bin/env python
"""The fused rotary embedding (llm_qat_amd.rope) beside the eager chain it replaces, on MI355X.

  shapes   bf16 q and k of [1, 32, 2048, 128] (7B), [1, 40, 2048, 128] (13B) and [4, 32, 2048, 128], both in the reference's transposed
           layout (views over [B, T, H * D] memory), gradients in the same layout, cached fp32 tables [1, 1, 2048, 128], position_ids [B, T];
           and the 7B shape with an fp32 k (..._k_fp32): what the reference runs under bf16 autocast with K/V quantization, where the
           chain promotes (fp32 results and incoming gradients; 7 bytes an element of q and k a phase instead of 4)
  eager    the reference's lines under bf16: the two casts of the cached tables (the rotary module's forward), the two squeezes and gathers
           and x * cos + rotate_half(x) * sin for q and k; then autograd's backward
  fused    rope.apply_rotary_pos_emb on the same arguments with the fp32 tables (rounded in the kernel): one kernel forward, one backward
  timing   HIP events around each phase, the two paths alternating call by call, the inputs rotated so that no call finds its tensors
           in the 256 MiB Infinity Cache; median and spread (min, max) over --iters calls after --warmup
  rates    event_time_bytes_per_s: the fused path's bytes (bytes_per_phase: each tensor read once, each result written once) over the EVENT time of a
           phase.  The event time holds the host's enqueue gaps, so this is the rate a caller sees, not a kernel's: the kernels' own
           rates come from a kernel trace (profiles/rope_kernel_times.txt)
  yardstick  fqa_swiglu_fwd (ops.swiglu_forward) on [rows, 4096] bf16 with rows chosen so that its 6 bytes per element equal the rotary
           forward's byte volume, timed the same way in the same process: what a streaming kernel of this library reaches at that size
  host     wall-clock time per forward-plus-backward call at a shape whose kernels take no time ([1, 2, 4, 16]), through the C++ node and
           through the Python Function: the host work in front of the two launches
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/rope_bench.py [--out profiles/rope_bench.json] [--iters 30] [--warmup 5] [--fused-only]

--fused-only leaves the eager chain and the host A/B out: for A/B runs of kernel variants (build.py -DROPE_NT_STORE=1
--out=..., then LLMQAT_AMD_LIB=... python tools/rope_bench.py --fused-only --out ...) and for kernel traces.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_qat_amd import _rope_node, ops, rope  # noqa: E402

# (B, H, T, D, dtype of k): bf16 q and k, and what the reference runs under bf16 autocast with K/V quantization: a bf16 q beside the fp32 k
# of its quantizer and fp32 tables, where the chain promotes (fp32 results and incoming gradients)
CASES = ((1, 32, 2048, 128, torch.bfloat16), (1, 40, 2048, 128, torch.bfloat16), (4, 32, 2048, 128, torch.bfloat16), (1, 32, 2048, 128, torch.float32))


def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def eager_rope(q, k, cos_cached, sin_cached, position_ids):
    """the rotary module's forward (the two casts of the cached tables, to the dtype of v, which is k's) and apply_rotary_pos_emb, as the
    reference runs them per layer"""
    t = q.shape[2]
    cos, sin = cos_cached[:, :, :t, ...].to(dtype=k.dtype), sin_cached[:, :, :t, ...].to(dtype=k.dtype)
    cos, sin = cos.squeeze(1).squeeze(0), sin.squeeze(1).squeeze(0)
    cos, sin = cos[position_ids].unsqueeze(1), sin[position_ids].unsqueeze(1)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def time_paths(paths, sets, tables, iters, warmup):
    """-> {name: (forward ms, backward ms)}, the paths alternating call by call"""
    out = {name: ([], []) for name, _ in paths}
    for i in range(warmup + iters):
        q, k, gq, gk, pos = sets[i % len(sets)]
        for name, fn in paths:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            qe, ke = fn(q, k, *tables, pos)
            e[1].record()
            torch.autograd.backward((qe, ke), (gq, gk))
            e[2].record()
            torch.cuda.synchronize()
            q.grad = k.grad = None
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


def peak(fn, q, k, gq, gk, pos, tables):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    qe, ke = fn(q, k, *tables, pos)
    torch.autograd.backward((qe, ke), (gq, gk))
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    q.grad = k.grad = None
    return out


def host_time(calls=300):
    """-> microseconds of wall clock per forward-plus-backward call at a shape whose kernels take no time, per node"""
    q = torch.randn(1, 4, 2 * 16, device="cuda", dtype=torch.bfloat16).view(1, 4, 2, 16).transpose(1, 2).requires_grad_(True)
    k = torch.randn(1, 4, 2 * 16, device="cuda", dtype=torch.bfloat16).view(1, 4, 2, 16).transpose(1, 2).requires_grad_(True)
    cos, sin = torch.randn(1, 1, 8, 16, device="cuda"), torch.randn(1, 1, 8, 16, device="cuda")
    pos = torch.arange(4, device="cuda").unsqueeze(0)
    g = torch.randn(1, 2, 4, 16, device="cuda", dtype=torch.bfloat16)
    out = {}
    load = _rope_node.load
    for name in ("c++", "python", "c++", "python"):            # alternating; the second round is the one kept
        _rope_node.load = load if name == "c++" else (lambda: None)
        try:
            if name == "c++" and load() is None:
                out[name] = None
                continue
            for n in (20, calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    qe, ke = rope.apply_rotary_pos_emb(q, k, cos, sin, pos)
                    torch.autograd.backward((qe, ke), (g, g))
                    q.grad = k.grad = None
                torch.cuda.synchronize()
                out[name] = round((time.perf_counter() - t0) / n * 1e6, 2)
        finally:
            _rope_node.load = load
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rope_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rope_bench needs the GPU: a timing taken elsewhere says nothing")
    from llm_qat_amd import _lib
    _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "node": "c++" if _rope_node.load() is not None else "python", "shapes": {}}
    for B, H, T, D, kdt in CASES:
        n = 2 * B * H * T * D                               # elements of q and k
        mixed = kdt is not torch.bfloat16
        rdt = kdt                                           # the dtype of the results and of their gradients: the promoted one
        nbytes = 7 * n if mixed else 4 * n                  # a phase's traffic: q 2 + 4 and k 4 + 4 bytes an element where k is fp32, else 2 + 2 each
        nsets = max(2, -(-(600 << 20) // (2 * nbytes)))     # q, k and their gradients of every set: more than twice the Infinity Cache in rotation
        gen = torch.Generator(device="cuda").manual_seed(B + H)
        mk = lambda dt: torch.randn((B, T, H * D), device="cuda", dtype=dt, generator=gen).view(B, T, H, D).transpose(1, 2)  # noqa: E731
        sets = [(mk(torch.bfloat16).requires_grad_(True), mk(kdt).requires_grad_(True), mk(rdt), mk(rdt), torch.arange(T, device="cuda").unsqueeze(0).expand(B, T).contiguous())
                for _ in range(nsets)]
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, device="cuda").float() / D))
        emb = torch.einsum("i,j->ij", torch.arange(T, device="cuda", dtype=inv.dtype), inv)
        emb = torch.cat((emb, emb), dim=-1)
        tables = (emb.cos()[None, None], emb.sin()[None, None])
        paths = (("fused", rope.apply_rotary_pos_emb),) + (() if args.fused_only else (("eager", eager_rope),))
        entry = {"elements_q_and_k": n, "q_dtype": "bfloat16", "k_dtype": str(kdt).replace("torch.", ""), "bytes_per_phase": nbytes, "input_sets": nsets}
        for name, (fwd, bwd) in time_paths(paths, sets, tables, args.iters, args.warmup).items():
            both = [a + b for a, b in zip(fwd, bwd)]
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "peak_bytes_over_inputs": peak(dict(paths)[name], *sets[0], tables)}
        f = entry["fused"]
        for phase in ("forward", "backward"):
            f[phase]["event_time_bytes_per_s"] = round(nbytes / (f[phase]["median_ms"] * 1e-3) / 1e12, 3) * 1e12
        if not args.fused_only:
            fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
            entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
            entry["speedup_forward"] = round(entry["eager"]["forward"]["median_ms"] / f["forward"]["median_ms"], 2)
            entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]       # the gate: the fused path's slowest call beats the eager chain's fastest
        rows = round(nbytes / 6 / 4096)                   # the yardstick: swiglu's forward at the rotary forward's byte volume
        ysets = [(torch.randn((rows, 4096), device="cuda", dtype=torch.bfloat16, generator=gen), torch.randn((rows, 4096), device="cuda", dtype=torch.bfloat16, generator=gen))
                 for _ in range(max(2, -(-(600 << 20) // (4 * rows * 4096))))]
        ms = time_calls(ops.swiglu_forward, ysets, args.iters, args.warmup)
        entry["yardstick_swiglu_forward"] = dict(summary(ms), shape=[rows, 4096], bytes=6 * rows * 4096, rope_forward_bytes=nbytes,
                                                 event_time_bytes_per_s=round(6 * rows * 4096 / (statistics.median(ms) * 1e-3) / 1e12, 3) * 1e12)
        del ysets
        result["shapes"][f"{B}x{H}x{T}x{D}" + ("_k_fp32" if mixed else "")] = entry
        del sets
        torch.cuda.empty_cache()
    if not args.fused_only:
        result["host_us_per_forward_plus_backward_call"] = host_time()
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    if not args.fused_only and not all(e["faster_beyond_spread"] for e in result["shapes"].values()):
        raise SystemExit("gate missed: at some shape the fused forward plus backward's slowest call is not faster than the eager chain's fastest")


if __name__ == "__main__":
    main()
