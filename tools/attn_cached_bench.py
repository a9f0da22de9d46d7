"""The decode attention over an in-place cache against today's decode step, section 30's protocol: HIP events
around single calls through the Python front-end, the variants alternating call by call in one process, input sets rotated past the
Infinity Cache, 40 calls, median (min - max) in microseconds.  At section 34's gated shape [8, 32/8, 1, 8192], D 128, bf16:

  cached      cached_decode_attention with uniform lengths Smax - 1: appends one row and attends to Smax keys
  decode      decode_attention on an already concatenated cache of Smax keys: the same bytes read (timed twice per round, as decode and
              decode_again: the difference of their medians is the spread a difference has to exceed)
  cat_decode  torch.cat of k and v (Smax - 1 rows and the new one) followed by decode: today's step
  ragged      cached with lengths spread evenly over [Smax / 8, Smax - 1]: recorded, not gated

    python tools/attn_cached_bench.py [--calls 40] [--out profiles/attn_cached_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_qat_amd import attention  # noqa: E402

B, H, HKV, T, SMAX, D = 8, 32, 8, 1, 8192, 128
CACHE_BYTES = 512 << 20


def make(dev):
    """-> {variant: call} over one set of tensors"""
    q = torch.randn(B, H, T, D, device=dev).bfloat16()
    kc, vc = (torch.randn(B, HKV, SMAX, D, device=dev).bfloat16() for _ in range(2))
    kn, vn = (torch.randn(B, HKV, T, D, device=dev).bfloat16() for _ in range(2))
    old = [t[:, :, :SMAX - T].contiguous() for t in (kc, vc)]
    uniform = torch.full((B,), SMAX - T, dtype=torch.int32, device=dev)
    ragged = torch.linspace(SMAX // 8, SMAX - T, B, device=dev).to(torch.int32)

    def decode():
        return attention.decode_attention(q, kc, vc, None, D)
    return {"cached": lambda: attention.cached_decode_attention(q, kn, vn, kc, vc, uniform, D), "decode": decode,
            "cat_decode": lambda: attention.decode_attention(q, torch.cat([old[0], kn], 2), torch.cat([old[1], vn], 2), None, D), "decode_again": decode,
            "ragged": lambda: attention.cached_decode_attention(q, kn, vn, kc, vc, ragged, D)}, int(ragged.sum()) + B * T


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attn_cached_bench.json"))
    args = ap.parse_args()
    cache = 2 * B * HKV * SMAX * D * 2      # bytes of k and v: what the kernel streams, and what a set must exceed the cache with
    # the set changes with every CALL, not every round: a variant that ran right behind another on the same caches found a part of them
    # in the Infinity Cache (the first run of this tool: decode behind cached 66.7 us, the same call behind cat_decode 77.8 us)
    sets = [make("cuda") for _ in range(max(3, -(-CACHE_BYTES // cache)))]
    names = list(sets[0][0])
    assert len(names) % len(sets), "every variant must meet every set"
    t = {n: [] for n in names}
    with torch.no_grad():
        for i in range(args.calls + 4):
            for j, n in enumerate(names):
                us = timed(sets[(i * len(names) + j) % len(sets)][0][n])
                if i >= 4:
                    t[n].append(us)
    us = {n: [statistics.median(x), min(x), max(x)] for n, x in t.items()}
    spread = abs(us["decode"][0] - us["decode_again"][0])
    out = dict(device=torch.cuda.get_device_name(0), protocol=__doc__.split("\n\n")[0], shape=[B, f"{H}/{HKV}", T, SMAX], D=D, calls=args.calls, us=us,
               cache_bytes=cache, decode_spread_us=spread, cached_minus_decode_us=us["cached"][0] - us["decode"][0],
               cat_decode_minus_cached_us=us["cat_decode"][0] - us["cached"][0], within_spread=us["cached"][0] - us["decode"][0] <= spread,
               ragged_key_share=sets[0][1] / (B * SMAX))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
