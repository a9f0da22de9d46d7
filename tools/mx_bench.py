#!/usr/bin/env python3
"""OCP MX block-scaled fake quantization on MI355X: HIP-event timings of fq_mx_fwd and fq_mx_export on a bf16 [4096, 11008] weight for each
format, against the per-channel Sym training forward (fq_sym_fwd_train) of the same tensor, and of a QuantizeLinear(4096 -> 11008)
forward + backward on 2048 bf16 tokens at MXFP4 weight / MXFP8-e4m3 activation against per-channel W4A8 and W4-g128.  The rotated forms
(fq_mx_fwd_rot, fq_mx_export_rot, fq_block_rotate, QuantizeLinear(mx_rotate=True), MXLinear(rotate=True) at 16 and
2048 tokens) are timed in the same rounds as their unrotated counterparts.  Writes JSON to profiles/ (or --out).

Method (tools/group_bench.py's): warm-up, then `--iters` launches per variant, variants alternated round by round, each launch reading a
different buffer from a rotation larger than the 256 MiB Infinity Cache, so every input comes from HBM.  The median of the rounds is
reported.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/mx_bench.py --quick` (a run of its own).

    python tools/mx_bench.py [--quick] [--out profiles/mx_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from group_bench import rotation, time_variants  # noqa: E402

PIN_TBPS = 8.0


def kernel_cases(shape, dtype, iters, rounds):
    from llm_qat_amd import _lib, ops
    xs = rotation(shape, dtype)
    n = len(xs)
    rows, cols = shape
    code = ops._DTYPES[dtype]
    L = _lib.lib()
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    el8 = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")
    el4 = torch.empty(rows * cols // 2, dtype=torch.uint8, device="cuda")
    sc = torch.empty(rows * cols // 32, dtype=torch.uint8, device="cuda")
    v = {}
    for name, f in ops.MX_FORMATS.items():     # the C entry points straight: no Python allocation in the timed loop
        v[f"fq_mx_fwd[{name}]"] = (lambda f: lambda i: _lib.check(L.fq_mx_fwd(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, f, code, None),
                                                                        "fq_mx_fwd"))(f)
    for name in ("mxfp4", "mxfp8_e4m3", "mxfp8_e5m2"):
        f = ops.MX_FORMATS[name]
        el = el4 if name == "mxfp4" else el8
        v[f"fq_mx_export[{name}]"] = (lambda f, el: lambda i: _lib.check(L.fq_mx_export(xs[i % n].data_ptr(), el.data_ptr(), sc.data_ptr(), rows, cols,
                                                                                                 f, code, None), "fq_mx_export"))(f, el)
    for name, f in ops.MX_FORMATS.items():     # the rotated forms, alternated with the unrotated ones above
        v[f"fq_mx_fwd_rot[{name}]"] = (lambda f: lambda i: _lib.check(L.fq_mx_fwd_rot(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, f, code,
                                                                                                None), "fq_mx_fwd_rot"))(f)
    for name in ("mxfp4", "mxfp8_e4m3"):
        f = ops.MX_FORMATS[name]
        el = el4 if name == "mxfp4" else el8
        v[f"fq_mx_export_rot[{name}]"] = (lambda f, el: lambda i: _lib.check(L.fq_mx_export_rot(xs[i % n].data_ptr(), el.data_ptr(), sc.data_ptr(), rows,
                                                                                                         cols, f, code, None), "fq_mx_export_rot"))(f, el)
    v["fq_block_rotate"] = lambda i: _lib.check(L.fq_block_rotate(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, code, None), "fq_block_rotate")
    v["fq_sym_fwd_train[w4]"] = lambda i: ops.quantize_train("sym", xs[i % n], 4, False, -2.0, 2.0)
    out = time_variants(v, iters, rounds)
    nb = rows * cols * xs[0].element_size()
    rates = {}
    for k, us in out.items():
        if k.startswith("fq_mx_fwd") or k == "fq_block_rotate":
            moved = 2 * nb
        elif k.startswith("fq_mx_export"):
            moved = nb + rows * cols // (2 if "mxfp4" in k else 1) + rows * cols // 32
        else:
            continue
        rates[k + "_TBps"] = round(moved / (us * 1e-6) / 1e12, 2)
        rates[k + "_of_pin"] = round(moved / (us * 1e-6) / 1e12 / PIN_TBPS, 3)
    out.update(rates)
    out["bytes_fwd"] = 2 * nb
    for name in ops.MX_FORMATS:                # the gate of section 15: the fused kernel under 2.0 x the unrotated one
        out[f"fq_mx_fwd_rot[{name}]_over_unrotated"] = round(out[f"fq_mx_fwd_rot[{name}]"] / out[f"fq_mx_fwd[{name}]"], 3)
    for name in ("mxfp4", "mxfp8_e4m3"):
        out[f"fq_mx_export_rot[{name}]_over_unrotated"] = round(out[f"fq_mx_export_rot[{name}]"] / out[f"fq_mx_export[{name}]"], 3)
    out["fq_block_rotate_over_fq_mx_fwd[mxfp4]"] = round(out["fq_block_rotate"] / out["fq_mx_fwd[mxfp4]"], 3)
    return out


def linear_step(kw):
    from llm_qat_amd.utils_quant import QuantizeLinear
    m = QuantizeLinear(4096, 11008, w_bits=4, a_bits=8, **kw).cuda().bfloat16()
    x = (torch.randn(2048, 4096, device="cuda")).bfloat16().requires_grad_(True)

    def step(i):
        m(x).sum().backward()
    return step


def mx_linear_call(tokens, rotate):
    from llm_qat_amd import MXLinear
    from llm_qat_amd.utils_quant import QuantizeLinear
    q = QuantizeLinear(4096, 11008, w_bits=4, a_bits=8, weight_format="mxfp4", act_format="mxfp8_e4m3", mx_rotate=rotate).cuda().bfloat16()
    m = MXLinear.from_quantize_linear(q)
    x = torch.randn(tokens, 4096, device="cuda").bfloat16()

    def call(i):
        with torch.no_grad():
            m(x)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_bench needs a GPU")
    iters, rounds = (10, 2) if args.quick else (50, 5)
    rec = {"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S"), "iters": iters, "rounds": rounds,
           "unit": "us per call", "pin_TBps": PIN_TBPS}
    rec["bf16_4096x11008"] = kernel_cases((4096, 11008), torch.bfloat16, iters, rounds)
    rec["quantize_linear_step_4096x11008_x2048"] = time_variants({
        "MXFP4-W/MXFP8_e4m3-A": linear_step({"weight_format": "mxfp4", "act_format": "mxfp8_e4m3"}),
        "MXFP4-W/MXFP8_e4m3-A rotated": linear_step({"weight_format": "mxfp4", "act_format": "mxfp8_e4m3", "mx_rotate": True}),
        "W4A8 per-channel": linear_step({}),
        "W4-g128/A8": linear_step({"weight_group_size": 128})}, max(iters // 5, 2), rounds)
    rec["mx_linear_4096x11008"] = time_variants({f"{t} tokens{' rotated' if r else ''}": mx_linear_call(t, r) for t in (16, 2048) for r in (False, True)},
                                                iters, rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
