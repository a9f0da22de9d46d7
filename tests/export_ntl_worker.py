"""The cross of the export kernels' launch-shape tests (tests/test_gpu_export_shapes.py), as functions the test file calls in its own
process and as a program it starts in a FRESH child interpreter with LLMQAT_FQ_NT_LOAD_MIN_MB=0: the library reads that variable once per
process, and no tensor of the case list is large enough to take the non-temporal load instantiation (`NTL = true`) otherwise.

    LLMQAT_FQ_NT_LOAD_MIN_MB=0 python tests/export_ntl_worker.py <out.json>

Test infrastructure: writes {"cases": n, "failures": [...]} and exits non-zero if any case differs from the oracle."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import export_cases as E  # noqa: E402
from group_ntl_worker import to_dev  # noqa: E402

# one fitting and one saturating combination per container, Sym and Asym: what the child interpreter runs at every 5-row shape
NTL_COMBOS = [E.Combo(k, b, c, False) for k in ("sym", "asym") for b, c in ((4, "int4"), (8, "int4"), (8, "int8"), (16, "int8"), (16, "int16"), (17, "int16"))]
NTL_DTYPES = ("bf16", "fp32")


def ntl_cases(dt):
    return [(c, sh) for sh in E.widths(dt) if sh.rows == 5 for c in NTL_COMBOS]


def export(x, c):
    from llm_qat_amd import ops
    if c.kind == "sym":
        return ops.sym_export(x, c.bits, container=c.container, autocast=c.autocast)
    return ops.asym_export(x, c.bits, container=c.container)


def raw_bytes(e, rows):
    return e.bins.contiguous().view(torch.uint8).reshape(rows, -1).cpu().numpy()


def compare(got_bytes, got_scales, got_over, want, c, what):
    """every packed byte, every scale as bits (Asym beta up to the sign of zero), every overflow count -> failure text or None"""
    wb, ws, wo = want
    bad = []
    if got_bytes.shape != wb.shape:
        return f"{what}: packed shape {got_bytes.shape} != {wb.shape}"
    d = got_bytes != wb
    if d.any():
        r, b = np.argwhere(d)[0]
        bad.append(f"{int(d.sum())} bytes differ (rows {sorted(set(np.nonzero(d)[0].tolist()))}), first row {r} byte {b}: got {got_bytes[r, b]:#04x} want {wb[r, b]:#04x}")
    if (got_over != wo).any():
        bad.append(f"overflow {got_over.tolist()} != {wo.tolist()}")
    if not E.scales_equal(got_scales, ws, c.kind == "asym"):
        bad.append(f"scales {np.asarray(got_scales).view(np.uint32).tolist()} != {np.asarray(ws).view(np.uint32).tolist()}")
    return f"{what}: " + "; ".join(bad) if bad else None


def run_cases(dt, cases, sem=None):
    """each (Combo, Shape) through ops.sym_export / ops.asym_export under the current semantics -> (cases run, failure texts); sem: the
    oracle's scalar policy for the expected values (None: the CPU policy, the device's under autocast)"""
    failures = []
    for c, sh in cases:
        x = to_dev(E.export_inputs(dt, *c, sh.cols, sh.rows), dt)
        e = export(x, c)
        r = E.RUNGS[sh.rung]
        msg = compare(raw_bytes(e, sh.rows), e.scales.cpu().numpy(), e.overflow.cpu().numpy(), E.expected(dt, *c, sh.cols, sh.rows, sem), c,
                      f"{dt} {c.kind} {c.bits} -> {c.container}{' autocast' if c.autocast else ''} at {r.tpr} x {r.vpt} ({sh.kind}, [{sh.rows}, {sh.cols}])")
        if msg:
            failures.append(msg)
    return len(cases), failures


def main(out):
    assert os.environ.get("LLMQAT_FQ_NT_LOAD_MIN_MB") == "0", "start this worker with LLMQAT_FQ_NT_LOAD_MIN_MB=0"
    import llm_qat_amd
    llm_qat_amd.set_semantics("cpu_eager")
    total, failures = 0, []
    for dt in NTL_DTYPES:
        n, f = run_cases(dt, ntl_cases(dt))
        total += n
        failures += f
    torch.cuda.synchronize()
    with open(out, "w") as fh:
        json.dump({"cases": total, "failures": failures[:20]}, fh)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
