"""A/B of kv_decode_attention against decode_attention on the equivalent 16-bit cache, section 30's protocol: HIP
events around single calls through the Python front-end, the two calls alternating call by call in one process, input sets rotated past
the Infinity Cache, 40 calls, median (min - max) in microseconds.

    python tools/attn_kvdecode_bench.py [--calls 40] [--out profiles/attn_kvdecode_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_qat_amd import attention, ops  # noqa: E402

ROWS = [(1, 32, 1, 2048, 128), (1, 32, 1, 8192, 128), (8, 32, 1, 2048, 128), (8, 32, 16, 2048, 128), (32, 32, 1, 512, 128), (8, 32, 1, 2048, 64),
        (8, 32, 1, 8192, 128)]      # [B, H, T, S], D: section 30's six rows and the long stream
STREAM = {(8, 32, 1, 2048, 128), (8, 32, 1, 8192, 128)}      # the gated, stream-bound rows
CACHE_BYTES = 512 << 20


def make(B, H, T, S, D, bits, rot, dev):
    per = 1 if bits == 8 else 2
    lo, hi = (-128, 128) if bits == 8 else (0, 256)
    a = dict(q=torch.randn(B, H, T, D, device=dev).bfloat16())
    for n in "kv":
        a[n + "_codes"] = torch.randint(lo, hi, (B, S, H, D // per), device=dev).to(torch.int8 if bits == 8 else torch.uint8).transpose(1, 2)
        a[n + "_t2"] = torch.rand(B, S, device=dev) * 40 + 20
    a["rotary"] = a["pos"] = None
    if rot:
        ang = torch.outer(torch.arange(S, device=dev).float(), 1.0 / 10000 ** (torch.arange(0, D, 2, device=dev).float() / D))
        a["rotary"] = tuple(f(torch.cat((ang, ang), -1)).bfloat16() for f in (torch.cos, torch.sin))
        a["pos"] = torch.arange(S, device=dev).expand(B, S).contiguous()
    a["k"] = ops.kv_codes_materialize(a["k_codes"], a["k_t2"], torch.bfloat16, bits, a["rotary"], a["pos"]).transpose(1, 2).contiguous().transpose(1, 2)
    a["v"] = ops.kv_codes_materialize(a["v_codes"], a["v_t2"], torch.bfloat16, bits).transpose(1, 2).contiguous().transpose(1, 2)
    return a


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attn_kvdecode_bench.json"))
    args = ap.parse_args()
    dev, rows = "cuda", []
    for B, H, T, S, D in ROWS:
        for bits in (8, 4):
            for rot in (False, True):
                wide = 2 * B * H * S * D * 2
                sets = [make(B, H, T, S, D, bits, rot, dev) for _ in range(max(2, min(16, -(-CACHE_BYTES // wide))))]
                t = {"codes": [], "wide": []}
                with torch.no_grad():
                    for i in range(args.calls + 4):
                        a = sets[i % len(sets)]
                        c = timed(lambda: attention.kv_decode_attention(a["q"], a["k_codes"], a["k_t2"], a["v_codes"], a["v_t2"], None, D, num_bits=bits,
                                                                        rotary=a["rotary"], key_positions=a["pos"]))
                        w = timed(lambda: attention.decode_attention(a["q"], a["k"], a["v"], None, D))
                        if i >= 4:
                            t["codes"].append(c)
                            t["wide"].append(w)
                med = {n: statistics.median(x) for n, x in t.items()}
                row = dict(shape=[B, H, T, S], D=D, bits=bits, rotary=rot, calls=args.calls, codes_us=[med["codes"], min(t["codes"]), max(t["codes"])],
                           wide_us=[med["wide"], min(t["wide"]), max(t["wide"])], ratio=med["wide"] / med["codes"], code_bytes=wide // 2 * bits // 8 // 1,
                           gated=(B, H, T, S, D) in STREAM and bits == 8, gate_met=med["codes"] < med["wide"])
                rows.append(row)
                print(json.dumps(row), flush=True)
                del sets
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), protocol=__doc__.split("\n\n")[0], rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
