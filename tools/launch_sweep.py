#!/usr/bin/env python3
"""One call per launch form of the host launch layer at small shapes, to see which kernel runs for which call.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/launch_sweep.py          # run the calls under the tracer
    python tools/launch_sweep.py --names <dir>                                                     # the ordered fq:: kernel names of a trace
    python tools/launch_sweep.py --families <dir>                                                  # the same condensed: hash + one line per template

Run it twice per library, the second time with LLMQAT_FQ_NT_LOAD_MIN_MB=0 (read once per process: every launch then takes the
non-temporal-load flavour), and once per library to compare (LLMQAT_AMD_LIB names another build): a change of the host layer that
leaves the selection alone gives the same ordered list of names.  Inputs are made on the CPU and copied, so PyTorch adds no kernels
between the calls; the results are not checked here (the test suite does that).

Per dtype: 5 rows at the tail width (lower bound + 1 vectors) of every rung of by_reg_shape -- forward plain, training, debug, Asym,
strided, pair, four tensors, autocast narrow and wide, every export container and the scale pre-pass; the group forward at every group
width on three rungs; every mask-backward form; fq_ste_bwd on aligned and odd lengths; both 1-/2-bit weight entry points; odd widths
for the generic kernels; [2, 40000] and [2, 40001] rows for the two passes; the MX forward, export, rotation, backward and GEMM."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNG_LOWER = (0, 64, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 2560, 3072, 3584, 4096, 5120, 6144, 7168)
LO, HI = -2.0, 2.0


def names(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "fq::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r["Kernel_Name"] for r in rows]


def families(kernel_names):
    """the ordered list condensed for reading: its SHA-256, then one line per kernel template -- dispatches, distinct instantiations, and
    each instantiation's template arguments (t / f for true / false) x its dispatches, in order of first appearance"""
    import hashlib
    import re
    fam = {}
    for n in kernel_names:
        m = re.match(r"(?:void )?fq::(\w+)(?:<(.*)>)?\(", n)
        args = (m.group(2) or "").replace("true", "t").replace("false", "f").replace(", ", ",")
        fam.setdefault(m.group(1), {}).setdefault(args, 0)
        fam[m.group(1)][args] += 1
    out = ["sha256 of the ordered list of %d names: %s" % (len(kernel_names), hashlib.sha256("\n".join(kernel_names).encode()).hexdigest())]
    for k, inst in fam.items():
        out.append("%s: %d dispatches, %d instantiations: %s" % (k, sum(inst.values()), len(inst), " ".join("<%s>x%d" % (a, c) for a, c in inst.items())))
    return out


def sweep():
    sys.path.insert(0, ROOT)
    import torch
    import llm_qat_amd
    from llm_qat_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    calls = [0]

    def t(rows, cols, dt):
        return (torch.randn(rows, cols, generator=gen) * 1.5).to(dt).to(dev)

    def ran(res):
        assert res is not None, "a form of the sweep was not served"
        calls[0] += 1
        return res

    for dt in (torch.bfloat16, torch.float16, torch.float32):
        epv = 4 if dt == torch.float32 else 8
        half = dt != torch.float32
        for lo in RUNG_LOWER:
            cols = (lo + 1) * epv
            x, w = t(5, cols, dt), t(3, cols, dt)
            ran(ops.sym_quantize(x, 4))
            ran(ops.train_forward("sym", x, 4, False, LO, HI))
            ran(ops.sym_quantize_debug(x, 4))
            ran(ops.asym_quantize(x, 4))
            ran(ops.train_forward("asym", x, 4, False, LO, HI))
            ran(ops.sym_quantize(t(5, 2 * cols, dt)[:, :cols], 4))
            ran(ops.pair_forward(w, x, 4, 8, LO, HI, True, True))
            ran(ops.multi_forward([x, w, t(2, cols, dt), t(1, cols, dt)], [8, 4, 4, 4], [True, True, False, True], LO, HI))
            if half:
                ran(ops.sym_forward_autocast(x, 8, False, False, LO, HI, train="mask"))
                ran(ops.sym_forward_autocast(x, 8, False, True, LO, HI, train="mask"))
                ran(ops.sym_forward_autocast(x, 8, False, True))
            for container in ("int4", "int8", "int16"):
                ran(ops.sym_export(x, 8, container=container, autocast=False))
            if half:
                ran(ops.sym_export(x, 8, container="int8", autocast=True))
            ran(ops.asym_export(x, 8, container="int8"))
            ran(ops.sym_row_scales(x, 8, autocast=False))
        for nvec in (128, 768, 4096):
            for gv in (4, 8, 16, 32, 64):
                x = t(5, nvec * epv, dt)
                ran(ops.group_forward("sym", x, 4, gv * epv))
                ran(ops.group_forward("asym", x, 4, gv * epv, train=True))
                if half:
                    ran(ops.group_forward("sym", x, 4, gv * epv, autocast=True))
        # the mask backwards: one copying tensor, in place, two slots, four slots, strided, behind a fp32-result forward
        for nvec in (65, 1025, 4095):      # (the fp32-gradient backward serves up to 32768 columns)
            cols = nvec * epv
            xs = [t(r, cols, dt) for r in (5, 3, 2, 1)]
            sides = [ran(ops.train_forward("sym", x, 4, False, LO, HI))[1] for x in xs]
            gs = [t(x.shape[0], cols, dt) for x in xs]
            ran(ops.train_backward(gs[0], sides[0], 5, cols, LO, HI))
            ran(ops.train_backward(gs[0].clone(), sides[0], 5, cols, LO, HI, inplace=True))
            ran(ops.pair_backward(gs[1], gs[0], sides[1], sides[0], 3, 5, cols, LO, HI))
            ran(ops.pair_backward(gs[1].clone(), gs[0], sides[1], sides[0], 3, 5, cols, LO, HI, inplace_w=True))
            ran(ops.multi_backward(list(gs), sides, [5, 3, 2, 1], cols, LO, HI))
            ran(ops.train_backward(t(5, 2 * cols, dt)[:, :cols], sides[0], 5, cols, LO, HI))
            if half:
                wide = [ran(ops.sym_forward_autocast(x, 8, False, True, LO, HI, train="mask"))[1] for x in xs[:2]]
                g32 = [t(x.shape[0], cols, torch.float32) for x in xs[:2]]
                ran(ops.train_backward_wide(g32[0], wide[0], 5, cols, LO, HI, dt))
                ran(ops.pair_backward_wide(g32[1], g32[0], wide[1], wide[0], 3, 5, cols, LO, HI, dt))
        for n in (4096, 4095):
            ran(ops.ste_backward(t(1, n, dt)[0], t(1, n, dt)[0], LO, HI))
        x = t(5, 520 * epv, dt)
        y, bounds = ran(ops.sym_quantize(x, 4, want_bounds=True))
        ran(ops.ste_backward(t(5, 520 * epv, dt), x, LO, HI, row_bounds=bounds, rows_cols_hint=(5, 520 * epv)))
        ran(ops.ste_backward(t(5, 1040 * epv, dt)[:, :520 * epv], x, LO, HI))
        for bits in (1, 2):
            for cols in (256, 255):
                w = (torch.randn(8, cols, generator=gen) * 1.5).to(dt)
                ran(ops.low_bit_weight(w.to(dev), w.abs().float().mean(1).to(dt).to(dev), bits))
            ran(ops.low_bit_weight_fused(t(8, 256, dt), bits))
            ran(ops.low_bit_weight_fused(t(8, 8192 + 64, dt), bits))
        for cols in (1001, 1027, 40000, 40001):      # the generic kernels either side of 1024 columns; the two passes
            x = t(2, cols, dt)
            ran(ops.sym_quantize(x, 4))
            ran(ops.asym_quantize(x, 4))
            if half:
                ran(ops.sym_forward_autocast(x, 8, False, False))
                ran(ops.sym_forward_autocast(x, 8, False, True))
            if cols < 40000:
                ran(ops.sym_export(x, 8, container="int8", autocast=False))
                ran(ops.asym_export(x, 8, container="int4"))
        x, g = t(64, 128, dt), t(64, 128, dt)
        for fmt in ops.MX_FORMATS:
            for rotate in (False, True):
                for rule in ops.MX_SCALE_RULES:
                    ran(ops.mx_quantize(x, fmt, rotate=rotate, scale_rule=rule))
                y, mask = ran(ops.mx_quantize(x, fmt, rotate=rotate, return_mask=True))
                ran(ops.mx_ste_backward(g, mask, rotate=rotate))
                if "fp6" not in fmt:
                    ran(ops.mx_export(x, fmt, rotate=rotate))
                    ran(ops.mx_export(x, fmt, rotate=rotate, scale_rule="ceil"))
        ran(ops.mx_rotate(x))
        for m in (8, 24, 64):          # the skinny GEMM's two forms and the tiled one
            for fa, fw in (("mxfp4", "mxfp4"), ("mxfp8_e4m3", "mxfp4"), ("mxfp8_e5m2", "mxfp8_e4m3")):
                ran(ops.mx_matmul(ops.mx_export(t(m, 128, dt), fa), ops.mx_export(t(32, 128, dt), fw)))
    c64 = torch.randn(5, 100, generator=gen, dtype=torch.float64) * 1.5
    x64 = c64.to(dev)
    ran(ops.sym_quantize(x64, 4))
    ran(ops.asym_quantize(x64, 4))
    ran(ops.ste_backward(x64.clone(), x64, LO, HI))
    for bits in (1, 2):
        ran(ops.low_bit_weight(x64, c64.abs().mean(1).to(dev), bits))
    torch.cuda.synchronize()
    from llm_qat_amd import _lib
    print("launch_sweep:", calls[0], "calls |", _lib.LIB_PATH, "| LLMQAT_FQ_NT_LOAD_MIN_MB =", os.environ.get("LLMQAT_FQ_NT_LOAD_MIN_MB"), "|", llm_qat_amd.__version__)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] in ("--names", "--families"):
        print("\n".join(names(sys.argv[2]) if sys.argv[1] == "--names" else families(names(sys.argv[2]))))
    else:
        sweep()
