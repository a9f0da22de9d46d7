"""The fused training attention beside the composed path it replaces (matmul, attn_softmax, matmul under autograd), forward plus
backward, on the GPU.

    python tools/attn_train_bench.py [--calls 20] [--out profiles/attn_train_bench.json]     timings, and the peak memory of both paths
    python tools/attn_train_bench.py --measure [--write]                                      the error measures over the tests' case list

Timings: HIP events around one forward plus backward through the Python front-end, the two paths alternating call by call in one
process, the input sets rotated so that q, k, v and dout of a call were last touched more than an Infinity Cache (256 MiB) ago; median
(min - max) over --calls calls after a warm-up of every shape.  bf16; under the fp32 causal mask the reference passes, without a mask,
and with causal=True (the composed path has no such mode: its row there is the fp32-mask one again).  The gate: under the fp32 mask the
fused median lies below the composed one and the two (min - max) ranges do not overlap.  Event times include the launch gaps of a
path's launches; kernel times come from a `rocprofv3 --kernel-trace` run of this script.
--measure: C_out, C_dq, C_dk, C_dv (tests/attn_train_reference.py) of both paths over DIMS x cases(); --write puts the composed path's
maxima, and the fused kernels' beside them, between the marker lines of that file.  No GPU: the script fails."""
import argparse
import json
import math
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llm_qat_amd import attention  # noqa: E402

SHAPES = [(1, 32, 2048, 2048, 128), (4, 32, 2048, 2048, 128), (1, 40, 2048, 2048, 128), (1, 32, 4096, 4096, 64)]
CACHE = 256 << 20


def composed(q, k, v, mask, D, causal=False):
    return torch.matmul(attention.attn_softmax(torch.matmul(q, k.transpose(2, 3)), mask, D), v)


def fused(q, k, v, mask, D, causal=False):
    return attention.train_attention(q, k, v, mask, D, causal=causal)


def step(fn, q, k, v, dout, mask, D, causal):
    return torch.autograd.grad(fn(q, k, v, mask, D, causal), (q, k, v), dout)


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step(fn, *a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stat(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def peak(fn, *a):
    """bytes allocated at the peak of one forward plus backward, over what the caller holds"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(fn, *a)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(calls, shapes):
    rows = []
    for si, (B, H, T, S, D) in enumerate(shapes):
        set_bytes = 2 * B * H * (2 * T + 2 * S) * D
        nsets = max(2, -(-2 * CACHE // set_bytes))
        sets = [tuple(torch.randn(B, H, n, D, device="cuda").bfloat16().requires_grad_(i < 3) for i, n in enumerate((T, S, S, T))) for _ in range(nsets)]
        causal = torch.zeros(B, 1, T, S, device="cuda").masked_fill(torch.ones(T, S, dtype=torch.bool, device="cuda").triu(S - T + 1), torch.finfo(torch.float32).min)
        for name, mask, flag in (("f32_causal", causal, False), ("none", None, False), ("causal_mode", None, True)):
            t = {"fused": [], "composed": []}
            for i in range(calls + 3):
                q, k, v, dout = sets[i % nsets]
                one = (timed(fused, q, k, v, dout, mask, D, flag), timed(composed, q, k, v, dout, causal if flag else mask, D, False))
                if i >= 3:
                    for key, us in zip(t, one):
                        t[key].append(us)
            row = {"shape": [B, H, T, S, D], "mask": name, **{key: stat(us) for key, us in t.items()}}
            row["gate_met"] = row["fused"]["median_us"] < row["composed"]["median_us"] and row["fused"]["max_us"] < row["composed"]["min_us"]
            if si == 0:
                row["peak_bytes"] = {"fused": peak(fused, *sets[0], mask, D, flag), "composed": peak(composed, *sets[0], causal if flag else mask, D, False)}
            print(json.dumps(row), flush=True)
            rows.append(row)
        del sets, causal
        torch.cuda.empty_cache()
    return rows


def measure():
    import attn_train_reference as R
    worst = {path: {n: (0.0, "") for n in R.NAMES} for path in ("composed", "fused")}
    for D, dtype, kind in R.DIMS:
        for T, S in R.cases(kind):
            q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, "cuda")
            dout = R.dout_of(T, D, dtype, "cuda")
            ref = R.ref64(q, k, v, ref_mask, R.inv_of(D), dout)
            for path, got in (("fused", R.fused(q, k, v, mask, D, dout, causal)), ("composed", R.composed(q, k, v, ref_mask, D, dout))):
                for n, c in R.measures(got, ref).items():
                    c = float("inf") if c != c else c      # a NaN would lose every comparison
                    worst[path][n] = max(worst[path][n], (c, f"D {D}, {str(dtype)[6:]}, {kind}, T {T}, S {S}"))
        print(D, dtype, kind, json.dumps(worst), flush=True)
    return worst


def write_measured(worst):
    path = os.path.join(ROOT, "tests", "attn_train_reference.py")
    lines = ["COMPOSED = {" + ", ".join(f'"{n}": {math.ceil(worst["composed"][n][0] * 1e4) / 1e4:.4f}' for n in worst["composed"]) + "}"]      # rounded up
    lines += [f"#   C_{n}: the composed path {worst['composed'][n][0]:.4f} ({worst['composed'][n][1]}); the fused kernels {worst['fused'][n][0]:.4f} "
              f"({worst['fused'][n][1]}), never part of the cap" for n in worst["composed"]]
    src = open(path).read()
    new = re.sub(r"(# -- measured [^\n]*\n).*?(# -- end measured --)", lambda m: m.group(1) + "\n".join(lines) + "\n" + m.group(2), src, flags=re.S)
    open(path, "w").write(new)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_train_bench.json"))
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, comma separated (default: all)")
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--write", action="store_true", help="with --measure: rewrite the measured block of tests/attn_train_reference.py")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    shapes = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    if args.measure:
        result = {"measures": measure()}
        if args.write:
            write_measured(result["measures"])
    else:
        result = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": bench(args.calls, shapes)}
    if not args.measure or args.out != ap.get_default("out"):
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
