#!/usr/bin/env python3
"""The MX block-scaled GEMM (fq_mx_gemm) on MI355X, HIP-event timings.

  skinny   M = 16 tokens, W mxfp4 [11008, 4096] and [4096, 11008], A mxfp8_e4m3: fq_mx_gemm against F.linear on the dequantized bf16
           weight; the achieved weight-byte rate (0.53 bytes per element) against the 6.29 TB/s copy figure.
  tiled    M = 2048 tokens, the LLaMA-7B projections 4096->11008, 11008->4096, 4096->4096, W/A = mxfp4/mxfp8_e4m3, mxfp4/mxfp4,
           mxfp8_e4m3/mxfp8_e4m3: TFLOP/s of the kernel, its ratio to the eval-mode fake-quant path on the same shapes (two fq_mx_fwd
           launches + the bf16 library GEMM), and end to end: MXLinear.forward against QuantizeLinear.eval() forward.
  accumulation error   max |out - ref| / (2^-24 * sum_k |a w|) per format pair against the float64 reference (bound: 2 K).

Method (tools/group_bench.py's): warm-up, `--iters` launches per variant, variants alternated round by round in one process, every launch
on the next weight of a rotation larger than the 256 MiB Infinity Cache; the median of the rounds is reported.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/mx_gemm_bench.py --quick` (a run of its own).

    python tools/mx_gemm_bench.py [--quick] [--out profiles/mx_gemm_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from group_bench import time_variants  # noqa: E402

COPY_TBPS = 6.29
IC_BYTES = 256 << 20
DT = torch.bfloat16


def _raw(L, a, w, out, M, N, K):
    from llm_qat_amd import _lib, ops
    return lambda: _lib.check(L.fq_mx_gemm(a.elements.data_ptr(), a.scales.data_ptr(), ops.MX_FORMATS[a.fmt], w.elements.data_ptr(),
                                           w.scales.data_ptr(), ops.MX_FORMATS[w.fmt], out.data_ptr(), M, N, K, ops._OUT_DTYPES[out.dtype], None),
                              "fq_mx_gemm")


def weights(N, K, fmt, bf16_too):
    """a rotation of exported weights past the Infinity Cache (and, for the bf16 baseline, of their dequantized bf16 forms)"""
    from llm_qat_amd import ops
    per = N * K // (2 if fmt == "mxfp4" else 1) + N * K // 32
    n = IC_BYTES // per + 2
    ex, dq = [], []
    for i in range(n):
        w = (torch.randn(N, K, device="cuda") * 0.02).to(DT)
        ex.append(ops.mx_export(w, fmt))
        if bf16_too and len(dq) * N * K * 2 <= IC_BYTES + N * K * 2:
            dq.append(ex[-1].dequantize())
    return ex, dq


def skinny(iters, rounds):
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    res = {}
    for N, K in ((11008, 4096), (4096, 11008)):
        M = 16
        ex, dq = weights(N, K, "mxfp4", True)
        x = torch.randn(M, K, device="cuda", dtype=DT)
        a = ops.mx_export(x, "mxfp8_e4m3")
        out = torch.empty(M, N, device="cuda", dtype=DT)
        calls = [_raw(L, a, w, out, M, N, K) for w in ex]
        v = {"fq_mx_gemm": lambda i: calls[i % len(calls)](),
             "F.linear_bf16": lambda i: F.linear(x, dq[i % len(dq)]),
             "export+mx_matmul": lambda i: ops.mx_matmul(ops.mx_export(x, "mxfp8_e4m3"), ex[i % len(ex)])}
        us = time_variants(v, iters, rounds)
        wbytes = N * K // 2 + N * K // 32
        res[f"M16_N{N}_K{K}"] = {"us": us, "rotation": {"mx_weights": len(ex), "bf16_weights": len(dq)},
                                 "mx_weight_bytes": wbytes, "mx_weight_TBps": round(wbytes / us["fq_mx_gemm"] / 1e6, 3),
                                 "share_of_copy_rate": round(wbytes / us["fq_mx_gemm"] / 1e6 / COPY_TBPS, 3),
                                 "bf16_weight_TBps": round(N * K * 2 / us["F.linear_bf16"] / 1e6, 3),
                                 "speedup_vs_bf16_linear": round(us["F.linear_bf16"] / us["fq_mx_gemm"], 3)}
        del ex, dq
    return res


def tiled(iters, rounds):
    from llm_qat_amd import MXLinear, _lib, ops
    from llm_qat_amd.utils_quant import QuantizeLinear
    L = _lib.lib()
    res = {}
    M = 2048
    for K, N in ((4096, 11008), (11008, 4096), (4096, 4096)):
        xs = [torch.randn(M, K, device="cuda", dtype=DT) for _ in range(3)]
        ws = [(torch.randn(N, K, device="cuda") * 0.02).to(DT) for _ in range(4)]
        out = torch.empty(M, N, device="cuda", dtype=DT)
        v = {}
        for wf, af in (("mxfp4", "mxfp8_e4m3"), ("mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp8_e4m3")):
            calls = [_raw(L, ops.mx_export(xs[i % 3], af), ops.mx_export(ws[i], wf), out, M, N, K) for i in range(4)]
            v[f"fq_mx_gemm[W {wf} / A {af}]"] = (lambda calls: lambda i: calls[i % 4]())(calls)
        v["parent_eval_path[2 fq_mx_fwd + bf16 GEMM]"] = lambda i: F.linear(ops.mx_quantize(xs[i % 3], "mxfp8_e4m3"), ops.mx_quantize(ws[i % 4], "mxfp4"))
        v["bf16_GEMM_alone"] = lambda i: F.linear(xs[i % 3], ws[i % 4])
        layer = QuantizeLinear(K, N, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3").to("cuda", DT).eval()
        mxl = MXLinear.from_quantize_linear(layer)
        with torch.no_grad():
            v["QuantizeLinear.eval().forward"] = lambda i: layer(xs[i % 3])
            v["MXLinear.forward"] = lambda i: mxl(xs[i % 3])
            us = time_variants(v, iters, rounds)
        flop = 2.0 * M * N * K
        r = {"us": us, "TFLOPs": {k: round(flop / t / 1e6, 1) for k, t in us.items() if k.startswith("fq_mx_gemm") or k == "bf16_GEMM_alone"}}
        r["kernel_vs_parent_eval_path"] = round(us["parent_eval_path[2 fq_mx_fwd + bf16 GEMM]"] / us["fq_mx_gemm[W mxfp4 / A mxfp8_e4m3]"], 3)
        r["MXLinear_vs_QuantizeLinear_eval"] = round(us["QuantizeLinear.eval().forward"] / us["MXLinear.forward"], 3)
        res[f"M{M}_{K}->{N}"] = r
    return res


def accumulation_error():
    from llm_qat_amd import ops
    res = {}
    fm = ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2")
    cpu = lambda e: ops.MXExport(e.elements.cpu(), e.scales.cpu(), e.fmt, e.shape, torch.float32).dequantize().double()
    for K in (4096, 11008):
        for af in fm:
            for wf in fm:
                worst = 0.0
                for M in (16, 160):
                    a = ops.mx_export(torch.randn(M, K, device="cuda"), af)
                    w = ops.mx_export(torch.randn(384, K, device="cuda") * 0.05, wf)
                    A, W = cpu(a), cpu(w)
                    err = (ops.mx_matmul(a, w, out_dtype=torch.float32).cpu().double() - A @ W.T).abs() / (2.0 ** -24 * (A.abs() @ W.abs().T))
                    worst = max(worst, err.max().item())
                res[f"A {af} x W {wf} K={K}"] = round(worst, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_gemm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx_gemm_bench: no GPU (timings are taken on the MI355X only)")
    torch.manual_seed(0)
    iters, rounds = (5, 2) if args.quick else (40, 7)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": iters, "rounds": rounds,
           "skinny": skinny(iters, rounds), "tiled": tiled(max(5, iters // 2), rounds)}
    if not args.quick:
        res["accumulation_error_over_2^-24_S"] = accumulation_error()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
