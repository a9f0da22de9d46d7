"""A/B of grouped-query attention against the same function on the expanded k, v, section 30's protocol: HIP events
around single calls through the Python front-end, the two calls alternating call by call in one process, input sets rotated past the
Infinity Cache, 40 calls, median (min - max) in microseconds.  The expansion is made outside the timed region.

    python tools/attn_gqa_bench.py [--calls 40] [--out profiles/attn_gqa_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_qat_amd import attention  # noqa: E402

D = 128
# (kernel, B, H, Hkv, T, S, rotary)
ROWS = [("decode", B, H, 8, T, S, False) for B, H, T in ((1, 32, 1), (8, 32, 1), (8, 64, 1)) for S in (2048, 8192)] + [("decode", 8, 32, 8, 4, 2048, False)] + \
       [("codes", 8, 32, 8, 1, 8192, rot) for rot in (False, True)] + [("codes", 8, 32, 8, 1, 2048, True)] + [("prefill", 1, 32, 8, 2048, 2048, False)]
GATED = {("decode", 8, 32, 8, 1, 2048, False), ("decode", 8, 32, 8, 1, 8192, False), ("codes", 8, 32, 8, 1, 2048, True), ("codes", 8, 32, 8, 1, 8192, True)}
CACHE_BYTES = 512 << 20


def make(kernel, B, H, Hkv, T, S, rot, dev):
    """-> (the grouped call, the call on the expanded cache, bytes of the grouped cache)"""
    G = H // Hkv
    q = torch.randn(B, H, T, D, device=dev).bfloat16()
    if kernel != "codes":
        k, v = (torch.randn(B, S, Hkv, D, device=dev).bfloat16().transpose(1, 2) for _ in range(2))
        kw, vw = (t.repeat_interleave(G, 1).transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
        fn = attention.decode_attention if kernel == "decode" else (lambda *a: attention.prefill_attention(*a, causal=True))
        return (lambda: fn(q, k, v, None, D)), (lambda: fn(q, kw, vw, None, D)), 2 * k.numel() * 2
    k, v = (torch.randint(-128, 128, (B, S, Hkv, D), device=dev).to(torch.int8).transpose(1, 2) for _ in range(2))
    kw, vw = (t.repeat_interleave(G, 1).transpose(1, 2).contiguous().transpose(1, 2) for t in (k, v))
    kt, vt = (torch.rand(B, S, device=dev) * 40 + 20 for _ in range(2))
    rotary = pos = None
    if rot:
        ang = torch.outer(torch.arange(S, device=dev).float(), 1.0 / 10000 ** (torch.arange(0, D, 2, device=dev).float() / D))
        rotary = tuple(f(torch.cat((ang, ang), -1)).bfloat16() for f in (torch.cos, torch.sin))
        pos = torch.arange(S, device=dev).expand(B, S).contiguous()

    def call(kc, vc):
        return lambda: attention.kv_decode_attention(q, kc, kt, vc, vt, None, D, rotary=rotary, key_positions=pos)
    return call(k, v), call(kw, vw), 2 * k.numel()


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attn_gqa_bench.json"))
    args = ap.parse_args()
    dev, rows = "cuda", []
    for row in ROWS:
        kernel, B, H, Hkv, T, S, rot = row
        wide = 2 * B * H * S * D * (1 if kernel == "codes" else 2)      # bytes of the expanded cache: what a set must exceed the cache with
        sets = [make(*row, dev) for _ in range(max(2, min(16, -(-CACHE_BYTES // wide))))]
        t = {"gqa": [], "expanded": []}
        with torch.no_grad():
            for i in range(args.calls + 4):
                g, w, nbytes = sets[i % len(sets)]
                tg, tw = timed(g), timed(w)
                if i >= 4:
                    t["gqa"].append(tg)
                    t["expanded"].append(tw)
        med = {n: statistics.median(x) for n, x in t.items()}
        out = dict(kernel=kernel, shape=[B, f"{H}/{Hkv}", T, S], D=D, rotary=rot, calls=args.calls, gqa_us=[med["gqa"], min(t["gqa"]), max(t["gqa"])],
                   expanded_us=[med["expanded"], min(t["expanded"]), max(t["expanded"])], ratio=med["expanded"] / med["gqa"], byte_ratio=H // Hkv,
                   cache_bytes=nbytes, gated=row in GATED, gate_met=med["gqa"] < med["expanded"])
        rows.append(out)
        print(json.dumps(out), flush=True)
        del sets
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), protocol=__doc__.split("\n\n")[0], rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
