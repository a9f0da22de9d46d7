"""Decode step over a K/V cache of integer codes: cached_kv_decode_attention beside kv_decode_attention.

    python tools/attn_cached_codes_bench.py [--reps 60] [--out profiles/attn_cached_codes_bench.json]

Shape [8, 32 / 8, 1, 8192], D = 128, bf16, int8 and int4, rotated.  Per container five paths, alternating call by call in one process,
each call on the next of several input sets whose caches together exceed the 256 MiB Infinity Cache, timed by events around the call:

  cached     this call: in-place caches of Smax = 8192 + 64 rows, every length 8191 (8192 keys seen)
  ragged     this call with the lengths spread evenly over 1024 .. 8191
  alone_a/b  kv_decode_attention alone on an already concatenated cache of 8192 keys with an already built mask and positions: unchanged
             code, the yardstick; measured as two paths, whose difference is the spread
  cat_loop   today's loop: the five torch.cat (two code tensors, two divisor rows, the positions) and kv_decode_attention

Medians with (min - max) in microseconds, one JSON document.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from llm_qat_amd import attention  # noqa: E402

B, H, HKV, T, S, D, PAD, DEV, DT = 8, 32, 8, 1, 8192, 128, 64, "cuda", torch.bfloat16


def make_set(bits, g):
    W, cdt, lo, hi = (D, torch.int8, -128, 128) if bits == 8 else (D // 2, torch.uint8, 0, 256)
    rnd = lambda *shape: torch.randint(lo, hi, shape, generator=g, dtype=torch.int16).to(cdt).to(DEV)      # noqa: E731
    t2 = lambda n: (32.0 + 64.0 * torch.rand((B, n), generator=g)).to(DEV)      # noqa: E731
    s = dict(q=torch.randn((B, H, T, D), generator=g).to(DT).to(DEV), kc=rnd(B, HKV, S + PAD, W), vc=rnd(B, HKV, S + PAD, W), ktc=t2(S + PAD), vtc=t2(S + PAD),
             kn=rnd(B, HKV, T, W), vn=rnd(B, HKV, T, W), ktn=t2(T), vtn=t2(T))
    s["full"] = (s["kc"][:, :, :S], s["ktc"][:, :S], s["vc"][:, :, :S], s["vtc"][:, :S])      # the concatenated cache, in place
    s["past"] = tuple(t.narrow(2 if t.dim() == 4 else 1, 0, S - T) for t in s["full"])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "attn_cached_codes_bench.json"))
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    cos, sin = (torch.randn((S + PAD, D), generator=g).to(DT).to(DEV) for _ in range(2))
    mask = torch.zeros((B, 1, T, S), dtype=DT, device=DEV)
    pos, pos_new = torch.arange(S - T, device=DEV)[None].expand(B, -1).contiguous(), torch.arange(S - T, S, device=DEV)[None].expand(B, -1).contiguous()
    pos_full = torch.arange(S, device=DEV)[None].expand(B, -1).contiguous()
    lens = {"cached": torch.full((B,), S - T, dtype=torch.int32, device=DEV),
            "ragged": torch.linspace(1024, S - T, B).to(torch.int32).to(DEV)}
    result = dict(shape=[B, f"{H}/{HKV}", T, S], D=D, dtype="bfloat16", reps=args.reps, unit="us", device=torch.cuda.get_device_name(0), containers={})
    for bits in (8, 4):
        nsets = 4 if bits == 8 else 7      # caches of a set: 136 / 68 MiB
        sets = [make_set(bits, g) for _ in range(nsets)]

        def cached(s, which):
            return attention.cached_kv_decode_attention(s["q"], s["kn"], s["ktn"], s["vn"], s["vtn"], s["kc"], s["ktc"], s["vc"], s["vtc"], lens[which], D,
                                                        num_bits=bits, rotary=(cos, sin))

        def alone(s):
            return attention.kv_decode_attention(s["q"], *s["full"], mask, D, num_bits=bits, rotary=(cos, sin), key_positions=pos_full)

        def cat_loop(s):
            kc, kt, vc, vt = (torch.cat((old, new), 2 if old.dim() == 4 else 1) for old, new in zip(s["past"], (s["kn"], s["ktn"], s["vn"], s["vtn"])))
            return attention.kv_decode_attention(s["q"], kc, kt, vc, vt, mask, D, num_bits=bits, rotary=(cos, sin), key_positions=torch.cat((pos, pos_new), 1))
        paths = {"cached": lambda s: cached(s, "cached"), "alone_a": alone, "cat_loop": cat_loop, "alone_b": alone, "ragged": lambda s: cached(s, "ragged")}
        times = {n: [] for n in paths}
        with torch.no_grad():
            for r in range(args.warmup + args.reps):
                for i, (name, fn) in enumerate(paths.items()):
                    s = sets[(r * len(paths) + i) % nsets]
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(s)
                    b.record()
                    b.synchronize()
                    if r >= args.warmup:
                        times[name].append(a.elapsed_time(b) * 1e3)
        row = {n: dict(median=round(statistics.median(t), 1), min=round(min(t), 1), max=round(max(t), 1)) for n, t in times.items()}
        result["containers"]["int8" if bits == 8 else "int4"] = row
        for n, v in row.items():
            print(f"int{bits} {n:9s} {v['median']:8.1f} us ({v['min']:.1f} - {v['max']:.1f})", flush=True)
        del sets
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
