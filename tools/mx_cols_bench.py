#!/usr/bin/env python3
"""The column-block MX quantizer (fqt_mx_fwd_cols) on MI355X, HIP-event timings.

  kernels   bf16 [4096, 11008], [11008, 4096], [2048, 4096], mxfp8_e4m3:
              cols        the new kernel (blocks down the columns), one launch
              rows        the row kernel (fq_mx_fwd_ex) on the same tensor: the same bytes, the rate this tensor streams at
              transposed  what there was before: transpose copy, row kernel, transpose copy back (three launches, three times the bytes)
            required: cols faster than transposed on every shape; cols / rows is recorded, not fixed in advance.
  layer     one QuantizeLinear(4096 -> 11008, mxfp4 / mxfp8_e4m3) forward + backward on 2048 bf16 tokens, with and without
            mx_backward_format="mxfp8_e4m3".

Method (tools/mx_gemm_bench.py's): warm-up, `--iters` launches per variant, variants alternated round by round in one process, every
launch on the next tensor of a rotation larger than the 256 MiB Infinity Cache; the median of the rounds is reported.  Kernel times: run
under `rocprofv3 --kernel-trace --stats -- python tools/mx_cols_bench.py --quick` (a run of its own).

    python tools/mx_cols_bench.py [--quick] [--out profiles/mx_cols_bench.json]
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
FMT = "mxfp8_e4m3"
SHAPES = ((4096, 11008), (11008, 4096), (2048, 4096))


def kernels(iters, rounds):
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    code, dt = ops.MX_FORMATS[FMT], ops._DTYPES[DT]
    res = {}
    for R, C in SHAPES:
        nbytes = R * C * 2
        n = IC_BYTES // nbytes + 2
        xs = [(torch.randn(R, C, device="cuda") * 0.05).to(DT) for _ in range(n)]
        ys = [torch.empty(R, C, device="cuda", dtype=DT) for _ in range(n)]

        def cols(i):
            _lib.check(L.fqt_mx_fwd_cols(xs[i % n].data_ptr(), ys[i % n].data_ptr(), R, C, code, dt, 0, None), "fqt_mx_fwd_cols")

        def rows(i):
            _lib.check(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % n].data_ptr(), None, R, C, code, dt, 0, None), "fq_mx_fwd_ex")

        def transposed(i):
            return ops.mx_quantize(xs[i % n].t().contiguous(), FMT).t().contiguous()

        want = transposed(0)
        cols(0)
        torch.cuda.synchronize()
        if not torch.equal(ys[0].view(torch.int16), want.view(torch.int16)):
            sys.exit(f"mx_cols_bench: the kernel and the transposed route differ on [{R}, {C}]")
        del want
        t = time_rounds({"cols": cols, "rows": rows, "transposed": transposed}, iters, rounds)
        us = {k: v["median"] for k, v in t.items()}
        res[f"bf16_{R}x{C}"] = {"us": us, "spread": t, "rotation": n, "bytes_moved_one_pass": 2 * nbytes,
                                 "cols_TBps": round(2 * nbytes / us["cols"] / 1e6, 3), "rows_TBps": round(2 * nbytes / us["rows"] / 1e6, 3),
                                 "cols_over_rows": round(us["cols"] / us["rows"], 3), "transposed_over_cols": round(us["transposed"] / us["cols"], 3),
                                 "cols_faster_than_transposed": us["cols"] < us["transposed"]}
        del xs, ys
    return res


def layer(iters, rounds):
    from llm_qat_amd.utils_quant import QuantizeLinear
    K, N, M = 4096, 11008, 2048
    xs = [torch.randn(M, K, device="cuda", dtype=DT, requires_grad=True) for _ in range(3)]
    gs = [torch.randn(M, N, device="cuda", dtype=DT) for _ in range(3)]
    v = {}
    for name, fb in (("backward_bf16", None), ("backward_mxfp8_e4m3", "mxfp8_e4m3")):
        m = QuantizeLinear(K, N, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_backward_format=fb).to("cuda", DT)

        def step(i, m=m):
            x = xs[i % 3]
            x.grad = None
            m.weight.grad = None
            m(x).backward(gs[i % 3])

        v[name] = step
    t = time_rounds(v, iters, rounds)
    us = {k: r["median"] for k, r in t.items()}
    return {"shape": f"{M} tokens, {K} -> {N}, bf16, W mxfp4 / A mxfp8_e4m3", "us": us, "spread": t,
            "mx_backward_over_bf16_backward": round(us["backward_mxfp8_e4m3"] / us["backward_bf16"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_cols_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx_cols_bench: no GPU (timings are taken on the MI355X only)")
    torch.manual_seed(0)
    iters, rounds = (5, 2) if args.quick else (40, 7)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": iters, "rounds": rounds, "format": FMT,
           "kernels": kernels(iters, rounds), "layer_step": layer(max(5, iters // 2), rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
