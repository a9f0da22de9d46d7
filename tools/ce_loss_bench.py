#!/usr/bin/env python
"""The fused language-model loss (llm_qat_amd.lm_loss.causal_lm_loss) beside the eager lines it replaces, on MI355X.

  shapes   [1, 2048, 32000] and [4, 2048, 32000] bf16 logits (one and four sequences of the 7B vocabulary), int64 labels
  fused    causal_lm_loss forward (the row kernel and the sum), backward (one kernel), and their sum
  eager    cross_entropy(logits[..., :-1, :].contiguous().view(-1, V), labels[..., 1:].contiguous().view(-1)) under
           torch.autocast("cuda", bf16), then .backward()
  timing   HIP events around each phase, the inputs rotated so that no call finds its logits in a cache; median and spread
           (min, max) over --iters calls after --warmup
  rates    the fused kernels' bytes per second against the 8 TB/s pin rate, counting 2 B/element forward (the logits once) and
           4 B/element backward (the logits again, the gradient written)
  memory   peak allocated bytes over the baseline with the inputs alive, both paths

    python tools/ce_loss_bench.py [--out profiles/ce_loss_bench.json] [--iters 30] [--warmup 5] [--fused-only]

--fused-only leaves the eager chain out: for A/B runs of kernel variants (build.py -DCE_FWD_VIF=2 -DCE_BWD_VIF=2 --out=..., then
LLMQAT_AMD_LIB=... python tools/ce_loss_bench.py --fused-only --out ...) and for kernel traces.
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
from llm_qat_amd.lm_loss import causal_lm_loss  # noqa: E402

PIN_RATE = 8.0e12   # bytes per second


def eager_loss(logits, labels):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        shift_logits = logits[..., :-1, :].contiguous()
        shift_labels = labels[..., 1:].contiguous()
        return F.cross_entropy(shift_logits.view(-1, logits.shape[-1]), shift_labels.view(-1))


def time_path(loss_fn, pairs, iters, warmup):
    """-> per-call milliseconds of the forward and of the backward"""
    fwd, bwd = [], []
    for i in range(warmup + iters):
        x, lab = pairs[i % len(pairs)]
        x.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = loss_fn(x, lab)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    return fwd, bwd


def peak(loss_fn, x, lab):
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss_fn(x, lab).backward()
    torch.cuda.synchronize()
    out = torch.cuda.max_memory_allocated() - base
    x.grad = None
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ce_loss_bench.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ce_loss_bench needs the GPU: a timing taken elsewhere says nothing")
    from llm_qat_amd import _lib
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "dtype": "bfloat16", "iters": args.iters,
              "library": os.path.relpath(_lib.LIB_PATH, ROOT), "shapes": {}}
    for shape in ((1, 2048, 32000), (4, 2048, 32000)):
        n = shape[0] * shape[1] * shape[2]
        sets = 4 if shape[0] == 1 else 2          # 131 MB / 524 MB of logits per set against 256 MiB of Infinity Cache
        g = torch.Generator(device="cuda").manual_seed(shape[0])
        pairs = []
        for _ in range(sets):
            x = torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g).mul_(3).requires_grad_(True)
            lab = torch.randint(0, shape[2], shape[:2], device="cuda", generator=g)   # no ignored label: every row is read and written
            pairs.append((x, lab))
        entry = {"elements": n, "input_sets": sets}
        for name, fn in (("fused", causal_lm_loss),) + (() if args.fused_only else (("eager", eager_loss),)):
            fwd, bwd = time_path(fn, pairs, args.iters, args.warmup)
            both = [a + b for a, b in zip(fwd, bwd)]
            entry[name] = {"forward": summary(fwd), "backward": summary(bwd), "forward_plus_backward": summary(both),
                           "peak_bytes_over_inputs": peak(fn, *pairs[0])}
        f = entry["fused"]
        f["forward"]["fraction_of_pin_rate"] = round(2 * n / (f["forward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        f["backward"]["fraction_of_pin_rate"] = round(4 * n / (f["backward"]["median_ms"] * 1e-3) / PIN_RATE, 3)
        with torch.no_grad():
            entry["loss_fused"] = float(causal_lm_loss(*pairs[0]))
        if not args.fused_only:
            fb, eb = f["forward_plus_backward"], entry["eager"]["forward_plus_backward"]
            entry["speedup_forward_plus_backward"] = round(eb["median_ms"] / fb["median_ms"], 2)
            entry["faster_beyond_spread"] = fb["max_ms"] < eb["min_ms"]
            with torch.no_grad():
                entry["loss_eager"] = float(eager_loss(*pairs[0]))
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
