#!/usr/bin/env python3
"""Group-wise fake quantization on MI355X: HIP-event timings of the group kernel against the row-wise kernel of the same tensor, against
the view route (the row-wise kernels on the [rows * C / g, g] view, forward + mask backward) and of the QuantizeLinear W4-g128 / A8 step
against the per-channel W4A8 step.  Writes JSON to profiles/ (or --out).

Method: warm-up, then `--iters` launches per variant, variants alternated round by round (`--rounds`), each launch reading a different
buffer set from a rotation larger than the 256 MiB Infinity Cache, so every input comes from HBM.  The median of the rounds is reported.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/group_bench.py --quick` (a run of its own).

    python tools/group_bench.py [--quick] [--out profiles/group_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROT_BYTES = 640 << 20    # buffer rotation > Infinity Cache (256 MiB)


def rotation(shape, dtype, scale=0.05):
    n = max(2, int(ROT_BYTES // (torch.Size(shape).numel() * torch.tensor([], dtype=dtype).element_size())) + 1)
    return [(torch.randn(shape, device="cuda") * scale).to(dtype) for _ in range(n)]


def time_variants(variants, iters, rounds, warmup=5):
    """variants: name -> fn(i) launching once on buffer set i.  -> name -> median microseconds per call"""
    return {k: v["median"] for k, v in time_rounds(variants, iters, rounds, warmup).items()}


def time_rounds(variants, iters, rounds, warmup=5):
    """the same loop, keeping the spread of the rounds: name -> {"median", "min", "max"} microseconds per call"""
    for fn in variants.values():
        for i in range(warmup):
            fn(i)
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            b.synchronize()
            res[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in res.items()}


def weight_cases(shape, dtype, groups, iters, rounds):
    from llm_qat_amd import ops
    xs = rotation(shape, dtype)
    n = len(xs)
    rows = shape[0]
    v = {}
    for g in groups:
        v[f"group_train_fwd_g{g}"] = (lambda g: lambda i: ops.quantize_train("sym", xs[i % n], 4, False, -2.0, 2.0, group_size=g))(g)
    v["row_train_fwd"] = lambda i: ops.quantize_train("sym", xs[i % n], 4, False, -2.0, 2.0)
    v["view_route_train_fwd_g128"] = lambda i: ops.quantize_train("sym", xs[i % n].view(-1, 128), 4, False, -2.0, 2.0)
    out = time_variants(v, iters, rounds)
    # backwards from the recorded side outputs (copying launch): full-row layout vs the view's per-group rows
    gs = rotation(shape, dtype, 1.0)
    sides_g = [ops.quantize_train("sym", xs[i % n], 4, False, -2.0, 2.0, group_size=128) for i in range(len(gs))]
    sides_v = [ops.quantize_train("sym", xs[i % n].view(-1, 128), 4, False, -2.0, 2.0) for i in range(len(gs))]
    m = len(gs)
    cols = shape[-1]
    out.update(time_variants({
        "group_bwd_mask_g128": lambda i: ops.ste_backward_mask(gs[i % m], -2.0, 2.0, sides_g[i % m][1], sides_g[i % m][2], rows, cols),
        "view_route_bwd_mask_g128": lambda i: ops.ste_backward_mask(gs[i % m].view(-1, 128), -2.0, 2.0, sides_v[i % m][1], sides_v[i % m][2],
                                                                    rows * cols // 128, 128),
    }, iters, rounds))
    out["group_fwd_plus_bwd_g128"] = round(out["group_train_fwd_g128"] + out["group_bwd_mask_g128"], 2)
    out["view_route_fwd_plus_bwd_g128"] = round(out["view_route_train_fwd_g128"] + out["view_route_bwd_mask_g128"], 2)
    nbytes = torch.Size(shape).numel() * xs[0].element_size() * 2
    out["group_train_fwd_g128_TBps"] = round(nbytes / (out["group_train_fwd_g128"] * 1e-6) / 1e12, 2)
    return out


def linear_step(grouped, iters, rounds):
    from llm_qat_amd.utils_quant import QuantizeLinear
    kw = {"weight_group_size": 128} if grouped else {}
    m = QuantizeLinear(4096, 11008, w_bits=4, a_bits=8, **kw).cuda().bfloat16()
    x = (torch.randn(2048, 4096, device="cuda")).bfloat16().requires_grad_(True)

    def step(i):
        m(x).sum().backward()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_bench needs a GPU")
    iters, rounds = (10, 2) if args.quick else (50, 5)
    rec = {"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S"), "iters": iters, "rounds": rounds, "unit": "us per call"}
    rec["bf16_4096x11008_w4"] = weight_cases((4096, 11008), torch.bfloat16, (64, 128, 256), iters, rounds)
    rec["fp16_4096x11008_w4"] = weight_cases((4096, 11008), torch.float16, (128,), iters, rounds)
    rec["fp32_4096x4096_w4"] = weight_cases((4096, 4096), torch.float32, (128,), iters, rounds)
    rec["bf16_2048x4096_act"] = weight_cases((2048, 4096), torch.bfloat16, (128,), iters, rounds)
    rec["quantize_linear_step_4096x11008_x2048"] = time_variants({"W4-g128/A8": linear_step(True, iters, rounds),
                                                                  "W4A8 per-channel": linear_step(False, iters, rounds)}, max(iters // 5, 2), rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
