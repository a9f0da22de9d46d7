"""The fused decode attention beside the composed path it replaces (matmul, attn_softmax, matmul), on the GPU.

    python tools/attn_decode_bench.py [--calls 40] [--out profiles/attn_decode_bench.json]     timings
    python tools/attn_decode_bench.py --measure                                                 C_out of both paths over the tests' case list

Timings: HIP events around single calls, the two paths alternating call by call in one process, the input sets rotated so that k and v
of a call were last touched more than an Infinity Cache (256 MiB) ago; median (min - max) over --calls calls after a warm-up of every
shape.  bf16; with the fp32 causal-with-past mask and without a mask.  Beside each shape: the k + v bytes over the fused call's time, and
fqa_swiglu_fwd (ops.swiglu_forward) reading the same number of bytes in the same process.  Event times include the launch gaps of a
path's launches; kernel times come from a `rocprofv3 --kernel-trace` run of this script.  No GPU: the script fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llm_qat_amd import attention, ops  # noqa: E402

SHAPES = [(1, 32, 1, 2048, 128), (1, 32, 16, 2048, 128), (1, 32, 1, 8192, 128), (8, 32, 1, 2048, 128), (1, 40, 1, 2048, 128), (1, 32, 1, 4096, 64)]
CACHE = 256 << 20


def composed(q, k, v, mask, D):
    return torch.matmul(attention.attn_softmax(torch.matmul(q, k.transpose(2, 3)), mask, D), v)


def fused(q, k, v, mask, D):
    return attention.decode_attention(q, k, v, mask, D)


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(*a)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stat(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def bench(calls):
    rows = []
    for B, H, T, S, D in SHAPES:
        kv_bytes = 2 * B * H * S * D * 2
        nsets = max(2, -(-2 * CACHE // kv_bytes))
        sets = [tuple(torch.randn(B, H, n, D, device="cuda").bfloat16() for n in (T, S, S)) for _ in range(nsets)]
        gate = [torch.randn(kv_bytes // 4 // 4096, 4096, device="cuda").bfloat16() for _ in range(2 * nsets)]
        causal = torch.zeros(B, 1, T, S, device="cuda").masked_fill(torch.ones(T, S, dtype=torch.bool, device="cuda").triu(S - T + 1), torch.finfo(torch.float32).min)
        for name, mask in (("f32_causal", causal), ("none", None)):
            t = {"fused": [], "composed": [], "swiglu": []}
            for i in range(calls + 5):
                q, k, v = sets[i % nsets]
                one = (timed(fused, q, k, v, mask, D), timed(composed, q, k, v, mask, D),
                       timed(ops.swiglu_forward, gate[2 * (i % nsets)], gate[2 * (i % nsets) + 1]))
                if i >= 5:
                    for key, us in zip(t, one):
                        t[key].append(us)
            row = {"shape": [B, H, T, S, D], "mask": name, "kv_bytes": kv_bytes, **{key: stat(us) for key, us in t.items()}}
            row["fused_kv_TBps"] = kv_bytes / row["fused"]["median_us"] / 1e6
            row["swiglu_read_TBps"] = kv_bytes / row["swiglu"]["median_us"] / 1e6
            row["gate_met"] = row["fused"]["median_us"] < row["composed"]["median_us"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        del sets, gate
    return rows


def measure():
    import attn_decode_reference as R
    worst = {"fused": (0.0, ""), "composed": (0.0, "")}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = R.key_counts(lambda S: ops.attn_decode_workspace(R.B, R.H, 1, 64, S, cus)[1])
    for D, dtype, kind in R.DIMS:
        for T in R.TS:
            for S in counts:
                q, k, v = R.inputs(T, S, D, dtype, "cuda")
                mask = R.mask_of(kind, T, S, dtype, "cuda", batch=R.B if S % 2 else 1, pad=S // 4)
                ref, mag = R.ref64(q, k, v, mask, R.inv_of(D))
                for name, fn in (("fused", fused), ("composed", composed)):
                    c = R.c_out(fn(q, k, v, mask, D), ref, mag)
                    worst[name] = max(worst[name], (c, f"D{D} {dtype} {kind} T{T} S{S}"))
        print(D, dtype, kind, json.dumps(worst), flush=True)
    return worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_decode_bench.json"))
    ap.add_argument("--measure", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    with torch.no_grad():
        result = {"c_out": measure()} if args.measure else {"calls": args.calls, "device": torch.cuda.get_device_name(0), "rows": bench(max(30, args.calls))}
    if not args.measure:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
