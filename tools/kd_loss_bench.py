#!/usr/bin/env python
"""The fused distillation loss (llm_qat_amd.distill.kd_kl_loss) beside the eager chain it replaces, on MI355X.

  shapes   [1, 2048, 32000] and [4, 2048, 32000] bf16 logits (one and four sequences of the 7B vocabulary)
  fused    kd_kl_loss forward (the row kernel and the sum), backward (one kernel), and their sum
  eager    F.kl_div(F.log_softmax(s, 2), F.softmax(t, 2), reduction="batchmean") under torch.autocast("cuda", bf16), then .backward()
  timing   HIP events around each phase, the input pairs rotated so that no call finds its logits in a cache; median and spread
           (min, max) over --iters calls after --warmup
  rates    the fused kernels' bytes per second against the 8 TB/s pin rate, counting 4 B/element forward (both logits once) and
           6 B/element backward (both again, the gradient written)
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/kd_loss_bench.py [--out profiles/kd_loss_bench.json] [--iters 30] [--warmup 5]
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
from llm_qat_amd.distill import kd_kl_loss  # noqa: E402

PIN_RATE = 8.0e12   # bytes per second


def eager_loss(s, t):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return F.kl_div(F.log_softmax(s, dim=2), F.softmax(t, dim=2), reduction="batchmean")


def time_path(loss_fn, pairs, iters, warmup):
    """-> per-call milliseconds of the forward and of the backward"""
    fwd, bwd = [], []
    for i in range(warmup + iters):
        s, t = pairs[i % len(pairs)]
        s.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = loss_fn(s, t)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    return fwd, bwd


def peak(loss_fn, s, t):
    s.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss_fn(s, t).backward()
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    s.grad = None
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kd_loss_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kd_loss_bench needs the GPU: a timing taken elsewhere says nothing")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters, "shapes": {}}
    for shape in ((1, 2048, 32000), (4, 2048, 32000)):
        n = shape[0] * shape[1] * shape[2]
        sets = 4 if shape[0] == 1 else 2          # 262 MB / 1 GB of logits per pair against 256 MiB of Infinity Cache
        g = torch.Generator(device="cuda").manual_seed(shape[0])
        pairs = [(torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g).mul_(3).requires_grad_(True),
                  torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g).mul_(3)) for _ in range(sets)]
        entry = {"elements": n, "input_sets": sets}
        for name, fn in (("fused", kd_kl_loss), ("eager", eager_loss)):
            fwd, bwd = time_path(fn, pairs, args.iters, args.warmup)
            both = [a + b for a, b in zip(fwd, bwd)]
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "peak_bytes_over_inputs": peak(fn, *pairs[0])}
        f = entry["fused"]
        f["forward"]["fraction_of_pin_rate"] = round(4 * n / (f["forward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        f["backward"]["fraction_of_pin_rate"] = round(6 * n / (f["backward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
        entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
        entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]
        with torch.no_grad():
            entry["loss_fused"], entry["loss_eager"] = float(kd_kl_loss(*pairs[0])), float(eager_loss(*pairs[0]))
        result["shapes"]["x".join(map(str, shape))] = entry
        del pairs
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
