#!/usr/bin/env python3
"""The MX dequantize kernel (fqi_mx_dequant) and MXLinear's dequantized route on MI355X, HIP-event timings.

  kernel   [4096, 11008], [11008, 4096], [4096, 4096]; mxfp4 and mxfp8_e4m3 to bf16: fqi_mx_dequant beside fq_mx_fwd on a bf16 tensor of
           the same shape in the same session, bytes moved per time for both (dequantize: code + scale bytes in, 2 bytes per element out;
           fq_mx_fwd: 2 in, 2 out).
  layer    the three LLaMA-7B projections, W mxfp4 / A mxfp8_e4m3, bf16, at 16 .. 2048 tokens: MXLinear on the GEMM route, MXLinear(
           dequant_above=0) and QuantizeLinear.eval(); from these the recommended dequant_above (mx_inference.DEQUANT_ABOVE_DEFAULT): the
           smallest measured token count above which the dequantized route beats the GEMM route on all three shapes by more than the runs'
           spread (its slowest round under the other's fastest), or None.
  policy   --variant NAME=PATH (repeatable): another build of the library (build.py -DMXD_NT_LOAD=0/1 -DMXD_NT_STORE=0/1 --out=PATH), timed
           in the same process beside the product build, kernel and layer: the load / store cache policy A/B.

Method (tools/mx_gemm_bench.py's): warm-up, `--iters` launches per variant, variants alternated round by round in one process, every launch
on the next weight of a rotation larger than the 256 MiB Infinity Cache; the median of the rounds with their min - max.

    python tools/mx_dequant_bench.py [--quick] [--variant l1s0=build_tmp/lib_l1s0.so ...] [--out profiles/mx_dequant_bench.json]
"""
import argparse
import ctypes
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
SHAPES = ((4096, 11008), (11008, 4096), (4096, 4096))          # [N, K] of a weight
TOKENS = (16, 32, 64, 128, 256, 512, 2048)


def _weights(N, K, count):
    return [(torch.randn(N, K, device="cuda") * 0.02).to(DT) for _ in range(count)]


def kernel(iters, rounds, libs):
    """libs: name -> bound library; "product" is the one the package loaded"""
    from llm_qat_amd import _lib, ops
    res = {}
    for N, K in SHAPES:
        ws = _weights(N, K, IC_BYTES // (N * K * 2) + 2)
        ys = [torch.empty_like(w) for w in ws]
        for fmt in ("mxfp4", "mxfp8_e4m3"):
            per = N * K // (2 if fmt == "mxfp4" else 1) + N * K // 32
            n = IC_BYTES // per + 2
            ex = [ops.mx_export(ws[i % len(ws)] * (1 + i // len(ws)), fmt) for i in range(n)]
            code, dt = ops.MX_FORMATS[fmt], _lib.DTYPE_BF16

            def dequant(L):
                return lambda i: _lib.check(L.fqi_mx_dequant(ex[i % n].elements.data_ptr(), ex[i % n].scales.data_ptr(), ys[i % len(ys)].data_ptr(),
                                                             N, K, code, dt, None), "fqi_mx_dequant")
            v = {f"fqi_mx_dequant[{name}]": dequant(L) for name, L in libs.items()}
            L0 = libs["product"]
            v["fq_mx_fwd"] = lambda i: _lib.check(L0.fq_mx_fwd(ws[i % len(ws)].data_ptr(), ys[i % len(ys)].data_ptr(), N, K, code, dt, None), "fq_mx_fwd")
            us = time_rounds(v, iters, rounds)
            moved = {k: (per + N * K * 2 if k.startswith("fqi") else N * K * 4) for k in us}
            res[f"{fmt}_{N}x{K}"] = {"us": us, "bytes": {"dequant_in": per, "dequant_out": N * K * 2, "fq_mx_fwd_in": N * K * 2, "fq_mx_fwd_out": N * K * 2},
                                     "rotation": {"exports": n, "bf16_tensors": len(ws)},
                                     "TBps": {k: {"median": round(moved[k] / r["median"] / 1e6, 3), "min": round(moved[k] / r["max"] / 1e6, 3),
                                                  "max": round(moved[k] / r["min"] / 1e6, 3)} for k, r in us.items()}}
            del ex
        del ws, ys
    return res


def layer(iters, rounds, libs, tokens):
    from llm_qat_amd import MXLinear, _lib
    from llm_qat_amd.utils_quant import QuantizeLinear
    res = {}
    L0 = libs["product"]
    for N, K in SHAPES:
        nq = IC_BYTES // (N * K * 2) + 2
        qs = [QuantizeLinear(K, N, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3").to("cuda", DT).eval() for _ in range(nq)]
        per = N * K // 2 + N * K // 32
        nm = IC_BYTES // per + 2
        gemm = [MXLinear.from_quantize_linear(qs[i % nq]) for i in range(nm)]
        deq = []
        for m in gemm:                                  # the same buffers behind the other route
            d = MXLinear(K, N, "mxfp4", "mxfp8_e4m3", device="cuda", dequant_above=0)
            d.weight_elements, d.weight_scales = m.weight_elements, m.weight_scales
            deq.append(d)

        def under(L, fn):                               # the package's launches through another build of the library
            def run(i):
                _lib._lib = L
                try:
                    fn(i)
                finally:
                    _lib._lib = L0
            return run
        for T in tokens:
            xs = [torch.randn(T, K, device="cuda", dtype=DT) for _ in range(3)]
            v = {"MXLinear[gemm]": lambda i: gemm[i % nm](xs[i % 3]),
                 "QuantizeLinear.eval()": lambda i: qs[i % nq](xs[i % 3])}
            for name, L in libs.items():
                v[f"MXLinear[dequant,{name}]"] = under(L, lambda i: deq[i % nm](xs[i % 3]))
            with torch.no_grad():
                us = time_rounds(v, iters, rounds)
            d, g, q = us["MXLinear[dequant,product]"], us["MXLinear[gemm]"], us["QuantizeLinear.eval()"]
            res[f"{K}->{N}_T{T}"] = {"us": us, "dequant_beats_gemm_beyond_spread": d["max"] < g["min"],
                                     "eval_over_dequant": round(q["median"] / d["median"], 3), "eval_over_gemm": round(q["median"] / g["median"], 3)}
        del qs, gemm, deq
    return res


def recommend(layers, tokens):
    """the smallest measured token count above which the dequantized route wins on every shape at every larger measured count, or None
    (nothing is said about counts below the smallest measured one)"""
    wins = {T: all(layers[f"{K}->{N}_T{T}"]["dequant_beats_gemm_beyond_spread"] for N, K in SHAPES) for T in tokens}
    best = None
    for j in range(len(tokens) - 2, -1, -1):            # tokens[j] qualifies when every larger measured count wins
        if not all(wins[T] for T in tokens[j + 1:]):
            break
        best = tokens[j]
    return best, wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations and token counts")
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library (cache-policy A/B)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_dequant_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mx_dequant_bench: no GPU (timings are taken on the MI355X only)")
    from llm_qat_amd import _lib
    torch.manual_seed(0)
    libs = {"product": _lib.lib()}
    for spec in args.variant:
        name, path = spec.split("=", 1)
        libs[name] = _lib._bind(ctypes.CDLL(os.path.abspath(path)))
    iters, rounds = (5, 3) if args.quick else (20, 7)
    tokens = (16, 2048) if args.quick else TOKENS
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": iters, "rounds": rounds, "libraries": list(libs),
           "kernel": kernel(iters, rounds, libs), "layer": layer(iters, rounds, libs, tokens)}
    best, wins = recommend(res["layer"], tokens)
    res["dequant_wins_on_all_shapes"] = {str(T): w for T, w in wins.items()}
    res["dequant_above_default"] = best
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
