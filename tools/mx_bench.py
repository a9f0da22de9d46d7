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

--rules times instead, in one process and alternated the same way, the mask-emitting forward (fq_mx_fwd_ex), the
masked backward (fq_mx_ste_bwd) and its rotated form against fq_mx_fwd; with --parent-lib, the existing entry points of this tree's
library against another build's (the parent commit's), the other build taken twice so that its own run-to-run scatter is on record; and a
QuantizeLinear step with mx_ste="clip" against the identity gradient.  --reference-stats needs no GPU: from the numpy reference alone, the
share of elements the floor rule masks and the quantization MSE of the ceil rule relative to floor, per format.

    python tools/mx_bench.py --rules [--parent-lib other.so] [--out profiles/mx_rules_bench.json]
    python tools/mx_bench.py --reference-stats [--out profiles/mx_rules_reference_stats.json]
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

from group_bench import rotation, time_rounds, time_variants  # noqa: E402

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


def rules_kernel_cases(shape, dtype, iters, rounds):
    """the new kernels against fq_mx_fwd on the same rotation of buffers"""
    from llm_qat_amd import _lib, ops
    xs = rotation(shape, dtype)
    n = len(xs)
    rows, cols = shape
    code, f = ops._DTYPES[dtype], ops.MX_FORMATS["mxfp4"]
    L = _lib.lib()
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    mask = torch.empty(rows * cols // 8, dtype=torch.uint8, device="cuda")
    _lib.check(L.fq_mx_fwd_ex(xs[0].data_ptr(), ys[0].data_ptr(), mask.data_ptr(), rows, cols, f, code, 0, None), "fq_mx_fwd_ex")
    ck = _lib.check
    v = {
        "fq_mx_fwd[mxfp4]": lambda i: ck(L.fq_mx_fwd(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, f, code, None), "fwd"),
        "fq_mx_fwd_ex[mxfp4]": lambda i: ck(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), None, rows, cols, f, code, 0, None), "fwd_ex"),
        "fq_mx_fwd_ex[mxfp4,ceil]": lambda i: ck(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), None, rows, cols, f, code, 2, None), "fwd_ex"),
        "fq_mx_fwd_ex[mxfp4,mask]": lambda i: ck(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), mask.data_ptr(), rows, cols, f, code, 0, None), "fwd_ex"),
        "fq_mx_fwd_ex[mxfp4,mask,rot]": lambda i: ck(L.fq_mx_fwd_ex(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), mask.data_ptr(), rows, cols, f, code, 1, None), "fwd_ex"),
        "fq_mx_fwd_rot[mxfp4]": lambda i: ck(L.fq_mx_fwd_rot(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, f, code, None), "fwd_rot"),
        "fq_mx_ste_bwd": lambda i: ck(L.fq_mx_ste_bwd(xs[i % n].data_ptr(), mask.data_ptr(), ys[i % 2].data_ptr(), rows, cols, code, 0, None), "ste"),
        "fq_mx_ste_bwd[rot]": lambda i: ck(L.fq_mx_ste_bwd(xs[i % n].data_ptr(), mask.data_ptr(), ys[i % 2].data_ptr(), rows, cols, code, 1, None), "ste"),
        "fq_block_rotate": lambda i: ck(L.fq_block_rotate(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, code, None), "rot"),
    }
    out = time_rounds(v, iters, rounds)
    nb = rows * cols * xs[0].element_size()
    base = out["fq_mx_fwd[mxfp4]"]["median"]
    for k, r in out.items():
        moved = 2 * nb + (rows * cols // 8 if "mask" in k or "ste" in k else 0)
        r["TBps"] = round(moved / (r["median"] * 1e-6) / 1e12, 2)
        r["over_fq_mx_fwd"] = round(r["median"] / base, 3)
        r["bytes_over_fq_mx_fwd"] = round(moved / (2 * nb), 4)
    return out


def ab_existing(shape, dtype, parent_lib, iters, rounds):
    """fq_mx_fwd / fq_mx_export / the *_rot entry points of this tree's library and of `parent_lib`, alternating; the parent twice"""
    import ctypes
    from llm_qat_amd import _lib, ops
    xs = rotation(shape, dtype)
    n = len(xs)
    rows, cols = shape
    code = ops._DTYPES[dtype]
    ys = [torch.empty_like(xs[0]) for _ in range(2)]
    el8 = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")
    sc = torch.empty(rows * cols // 32, dtype=torch.uint8, device="cuda")
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    P = ctypes.CDLL(parent_lib)
    for name in ("fq_mx_fwd", "fq_mx_fwd_rot"):
        getattr(P, name).argtypes = [vp, vp, i64, i64, i32, i32, vp]
    for name in ("fq_mx_export", "fq_mx_export_rot"):
        getattr(P, name).argtypes = [vp, vp, vp, i64, i64, i32, i32, vp]
    libs = {"this": _lib.lib(), "parent": P, "parent_again": P}
    v = {}
    for fmt in ("mxfp4", "mxfp8_e4m3"):
        f = ops.MX_FORMATS[fmt]
        for tag, L in libs.items():
            for name in ("fq_mx_fwd", "fq_mx_fwd_rot"):
                v[f"{name}[{fmt}] {tag}"] = (lambda fn, f: lambda i: fn(xs[i % n].data_ptr(), ys[i % 2].data_ptr(), rows, cols, f, code, None))(getattr(L, name), f)
            for name in ("fq_mx_export", "fq_mx_export_rot"):
                v[f"{name}[{fmt}] {tag}"] = (lambda fn, f: lambda i: fn(xs[i % n].data_ptr(), el8.data_ptr(), sc.data_ptr(), rows, cols, f, code, None))(getattr(L, name), f)
    out = time_rounds(v, iters, rounds)
    summary = {}
    for k in [k[:-5] for k in out if k.endswith(" this")]:
        t, p, p2 = out[k + " this"]["median"], out[k + " parent"]["median"], out[k + " parent_again"]["median"]
        summary[k] = {"this_us": t, "parent_us": p, "parent_again_us": p2, "this_over_parent": round(t / p, 4),
                      "parent_scatter": round(abs(p - p2) / p, 4),
                      "parent_round_spread": round((out[k + " parent"]["max"] - out[k + " parent"]["min"]) / p, 4)}
    return {"rounds": out, "summary": summary}


def reference_stats():
    """numpy reference only: share of elements masked under floor, and MSE(ceil) / MSE(floor), on Gaussian and outlier-channel data"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mx_rules_reference as R
    from mx_reference import decode
    rng = np.random.default_rng(0)
    rows, cols = 512, 4096
    gauss = rng.standard_normal((rows, cols)).astype(np.float32)
    outl = gauss.copy()
    outl[:, rng.choice(cols, cols // 128, replace=False)] *= 30.0        # 1 channel in 128 carries 30 x the scale (section 15's data)
    rec = {"shape": [rows, cols], "dtype": "fp32", "data": {}}
    for dname, x in (("gaussian", gauss), ("outlier_channels", outl)):
        b = x.view(np.uint32)
        xv = x.astype(np.float64)
        rec["data"][dname] = {}
        for fmt in R.FORMATS:
            for rot in (False, True):
                src = R._source_bits(b, "fp32", rot)[0]
                xr = decode(src, "fp32") if rot else xv
                keep = R.keep_mask(b, "fp32", fmt, "floor", rot)
                mse = {rule: float(np.mean((R.quantize_values(b, "fp32", fmt, rule, rot) - xr) ** 2)) for rule in R.RULES}
                blocks = (~keep).reshape(-1, 32).any(1)
                rec["data"][dname][fmt + (" rotated" if rot else "")] = {
                    "masked_share_floor": float((~keep).mean()), "blocks_with_a_masked_element_floor": float(blocks.mean()),
                    "mse_floor": mse["floor"], "mse_ceil": mse["ceil"], "mse_ceil_over_floor": mse["ceil"] / mse["floor"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer iterations (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--rules", action="store_true", help="the scale-rule / saturation-mask measurements of DESIGN.md section 16")
    ap.add_argument("--parent-lib", default=None, help="with --rules: another build of the library to A/B the existing entry points against")
    ap.add_argument("--reference-stats", action="store_true", help="numpy reference only (no GPU): masked share and MSE of the scale rules")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reference_stats:
        rec = reference_stats()
        out = args.out or os.path.join(ROOT, "profiles", "mx_rules_reference_stats.json")
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return
    if args.rules:
        if not torch.cuda.is_available():
            raise SystemExit("mx_bench needs a GPU")
        iters, rounds = (10, 3) if args.quick else (50, 7)
        rec = {"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S"), "iters": iters, "rounds": rounds,
               "unit": "us per call"}
        rec["bf16_4096x11008"] = rules_kernel_cases((4096, 11008), torch.bfloat16, iters, rounds)
        if args.parent_lib:
            rec["existing_entry_points_vs_parent_bf16_4096x11008"] = ab_existing((4096, 11008), torch.bfloat16, args.parent_lib, iters, rounds)
        mx = {"weight_format": "mxfp4", "act_format": "mxfp8_e4m3"}
        rec["quantize_linear_step_4096x11008_x2048"] = time_rounds({
            "identity": linear_step(dict(mx)), "clip": linear_step(dict(mx, mx_ste="clip")),
            "identity ceil": linear_step(dict(mx, mx_scale_rule="ceil")), "clip ceil": linear_step(dict(mx, mx_ste="clip", mx_scale_rule="ceil")),
            "identity rotated": linear_step(dict(mx, mx_rotate=True)), "clip rotated": linear_step(dict(mx, mx_rotate=True, mx_ste="clip"))},
            max(iters // 5, 2), rounds)
        out = args.out or os.path.join(ROOT, "profiles", "mx_rules_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(rec))
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "mx_bench.json")
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
