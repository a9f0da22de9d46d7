"""The fused prefill attention beside the composed path it replaces (matmul, attn_softmax, matmul), on the GPU.

    python tools/attn_prefill_bench.py [--calls 20] [--out profiles/attn_prefill_bench.json]     timings
    python tools/attn_prefill_bench.py --measure                                                  C_out of both paths over the tests' case list

Timings: HIP events around single calls through the Python front-end, the two paths alternating call by call in one process, the input
sets rotated so that q, k and v of a call were last touched more than an Infinity Cache (256 MiB) ago; median (min - max) over --calls
calls after a warm-up of every shape.  bf16; with the fp32 causal mask the reference passes, without a mask, and with causal=True (the
composed path has no such mode: its row there is the fp32-mask one again).  Beside each row: the matrix work of the two products (4 B H T
S D FLOP; under a causal rule half of it is needed) over the fused call's time.  Event times include the launch gaps of a path's launches;
kernel times come from a `rocprofv3 --kernel-trace` run of this script.  No GPU: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llm_qat_amd import attention  # noqa: E402

SHAPES = [(1, 32, 2048, 2048, 128), (4, 32, 2048, 2048, 128), (1, 40, 2048, 2048, 128), (1, 32, 4096, 4096, 64), (1, 32, 64, 4096, 128)]
CACHE = 256 << 20


def composed(q, k, v, mask, D, causal=False):
    return torch.matmul(attention.attn_softmax(torch.matmul(q, k.transpose(2, 3)), mask, D), v)


def fused(q, k, v, mask, D, causal=False):
    return attention.prefill_attention(q, k, v, mask, D, causal=causal)


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stat(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def bench(calls, shapes):
    rows = []
    for B, H, T, S, D in shapes:
        set_bytes = 2 * B * H * (T + 2 * S) * D
        nsets = max(2, -(-2 * CACHE // set_bytes))
        sets = [tuple(torch.randn(B, H, n, D, device="cuda").bfloat16() for n in (T, S, S)) for _ in range(nsets)]
        causal = torch.zeros(B, 1, T, S, device="cuda").masked_fill(torch.ones(T, S, dtype=torch.bool, device="cuda").triu(S - T + 1), torch.finfo(torch.float32).min)
        for name, mask, flag in (("f32_causal", causal, False), ("none", None, False), ("causal_mode", None, True)):
            t = {"fused": [], "composed": []}
            for i in range(calls + 3):
                q, k, v = sets[i % nsets]
                one = (timed(fused, q, k, v, mask, D, flag), timed(composed, q, k, v, causal if flag else mask, D))
                if i >= 3:
                    for key, us in zip(t, one):
                        t[key].append(us)
            row = {"shape": [B, H, T, S, D], "mask": name, "flop": 4 * B * H * T * S * D, **{key: stat(us) for key, us in t.items()}}
            row["fused_TFLOPs"] = row["flop"] / row["fused"]["median_us"] / 1e6
            row["gate_met"] = row["fused"]["median_us"] < row["composed"]["median_us"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        del sets, causal
        torch.cuda.empty_cache()
    return rows


def measure():
    import attn_prefill_reference as R
    worst = {"fused": (0.0, ""), "composed": (0.0, "")}
    for D, dtype, kind in R.DIMS:
        for T, S in R.cases(kind):
            q, k, v, mask, causal, ref_mask = R.case_args(kind, T, S, D, dtype, "cuda")
            ref, mag = R.ref64(q, k, v, ref_mask, R.inv_of(D))
            for name, out in (("fused", fused(q, k, v, mask, D, causal)), ("composed", composed(q, k, v, ref_mask, D))):
                worst[name] = max(worst[name], (R.c_out(out, ref, mag), f"D{D} {dtype} {kind} T{T} S{S}"))
        print(D, dtype, kind, json.dumps(worst), flush=True)
    return worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_prefill_bench.json"))
    ap.add_argument("--shapes", default=None, help="indices into SHAPES, comma separated (default: all)")
    ap.add_argument("--measure", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    shapes = SHAPES if args.shapes is None else [SHAPES[int(i)] for i in args.shapes.split(",")]
    with torch.no_grad():
        result = {"c_out": measure()} if args.measure else {"calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": bench(args.calls, shapes)}
    if not args.measure:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
