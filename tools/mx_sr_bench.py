#!/usr/bin/env python3
"""MX fake quantization with stochastic rounding (fqs_mx_fwd / fqs_mx_fwd_cols) on MI355X, HIP-event timings.

  kernels   bf16 [4096, 11008], [11008, 4096], [2048, 4096], mxfp4 and mxfp8_e4m3:
              sr_rows / rows   the stochastic row kernel against the nearest one (fq_mx_fwd_ex) on the same tensors
              sr_cols / cols   the stochastic column kernel against the nearest one (fqt_mx_fwd_cols)
            sr / nearest is recorded, not fixed in advance: it is what the Philox4x32-10 call per eight elements costs a streaming kernel.
  pair      bf16 [4096, 11008]: one sr_rows launch against torch.rand_like(x) followed by the nearest row kernel -- the cheapest
            two-launch composition there is in place of the kernel (and it does not even compute its result).  Required: sr_rows faster.
  layer     one QuantizeLinear(4096 -> 11008, mxfp4 / mxfp8_e4m3) forward + backward on 2048 bf16 tokens with mx_backward_format="mxfp4",
            nearest against stochastic.

Method (tools/mx_cols_bench.py's): warm-up, `--iters` launches per variant, variants alternated round by round in one process, every
launch on the next tensor of a rotation larger than the 256 MiB Infinity Cache; median (min - max) of the rounds.

    python tools/mx_sr_bench.py [--quick] [--out profiles/mx_sr_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from group_bench import time_rounds  # noqa: E402

IC_BYTES = 256 << 20
DT = torch.bfloat16
FMTS = ("mxfp4", "mxfp8_e4m3")
SHAPES = ((4096, 11008), (11008, 4096), (2048, 4096))
PAIR_SHAPE = (4096, 11008)
SEED = 0x5EED0123456789AB


def kernels(iters, rounds):
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    dt = ops._DTYPES[DT]
    res = {}
    for R, C in SHAPES:
        nbytes = R * C * 2
        n = IC_BYTES // nbytes + 2
        xs = [(torch.randn(R, C, device="cuda") * 0.05).to(DT) for _ in range(n)]
        ys = [torch.empty(R, C, device="cuda", dtype=DT) for _ in range(n)]
        for fmt in FMTS:
            code = ops.MX_FORMATS[fmt]

            def sr_rows(i):
                _lib.check(L.fqs_mx_fwd(xs[i % n].data_ptr(), ys[i % n].data_ptr(), R, C, code, dt, 0, SEED, i, None), "fqs_mx_fwd")

            def rows(i):
                _lib.check(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % n].data_ptr(), None, R, C, code, dt, 0, None), "fq_mx_fwd_ex")

            def sr_cols(i):
                _lib.check(L.fqs_mx_fwd_cols(xs[i % n].data_ptr(), ys[i % n].data_ptr(), R, C, code, dt, 0, SEED, i, None), "fqs_mx_fwd_cols")

            def cols(i):
                _lib.check(L.fqt_mx_fwd_cols(xs[i % n].data_ptr(), ys[i % n].data_ptr(), R, C, code, dt, 0, None), "fqt_mx_fwd_cols")

            v = {"sr_rows": sr_rows, "rows": rows, "sr_cols": sr_cols, "cols": cols}
            if (R, C) == PAIR_SHAPE:
                def rand_then_rows(i):
                    torch.rand_like(xs[i % n])
                    rows(i)
                v["rand_like_then_rows"] = rand_then_rows
            t = time_rounds(v, iters, rounds)
            us = {k: r["median"] for k, r in t.items()}
            entry = {"us": us, "spread": t, "rotation": n, "bytes_moved_one_pass": 2 * nbytes,
                     "sr_rows_TBps": round(2 * nbytes / us["sr_rows"] / 1e6, 3), "rows_TBps": round(2 * nbytes / us["rows"] / 1e6, 3),
                     "sr_cols_TBps": round(2 * nbytes / us["sr_cols"] / 1e6, 3), "cols_TBps": round(2 * nbytes / us["cols"] / 1e6, 3),
                     "sr_rows_over_rows": round(us["sr_rows"] / us["rows"], 3), "sr_cols_over_cols": round(us["sr_cols"] / us["cols"], 3)}
            if (R, C) == PAIR_SHAPE:
                entry["sr_rows_over_rand_like_then_rows"] = round(us["sr_rows"] / us["rand_like_then_rows"], 3)
                entry["sr_rows_faster_than_rand_like_then_rows"] = t["sr_rows"]["median"] < t["rand_like_then_rows"]["median"]
            res[f"bf16_{R}x{C}_{fmt}"] = entry
        del xs, ys
    return res


def layer(iters, rounds):
    import llm_qat_amd
    from llm_qat_amd.utils_quant import QuantizeLinear
    K, N, M = 4096, 11008, 2048
    xs = [torch.randn(M, K, device="cuda", dtype=DT, requires_grad=True) for _ in range(3)]
    gs = [torch.randn(M, N, device="cuda", dtype=DT) for _ in range(3)]
    llm_qat_amd.mx_sr_seed(SEED)
    v = {}
    for name in ("nearest", "stochastic"):
        m = QuantizeLinear(K, N, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_backward_format="mxfp4",
                           mx_backward_rounding=name).to("cuda", DT)

        def step(i, m=m):
            x = xs[i % 3]
            x.grad = None
            m.weight.grad = None
            m(x).backward(gs[i % 3])

        v[name] = step
    t = time_rounds(v, iters, rounds)
    us = {k: r["median"] for k, r in t.items()}
    return {"shape": f"{M} tokens, {K} -> {N}, bf16, W mxfp4 / A mxfp8_e4m3, backward mxfp4", "us": us, "spread": t,
            "stochastic_over_nearest": round(us["stochastic"] / us["nearest"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_sr_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx_sr_bench: no GPU (timings are taken on the MI355X only)")
    torch.manual_seed(0)
    iters, rounds = (5, 2) if args.quick else (40, 7)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": iters, "rounds": rounds, "formats": list(FMTS),
           "kernels": kernels(iters, rounds), "layer_step": layer(max(5, iters // 2), rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
