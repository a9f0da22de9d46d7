"""The plain-mode cross of the group-wise kernel's launch-shape tests (tests/test_gpu_group_shapes.py), as a function the test file calls
in its own process and as a program it starts in a FRESH child interpreter with LLMQAT_FQ_NT_LOAD_MIN_MB=0: the library reads that
variable once per process, and no tensor of the case list is large enough to take the non-temporal load branch (`ga.ntl`) otherwise.

    LLMQAT_FQ_NT_LOAD_MIN_MB=0 python tests/group_ntl_worker.py <out.json>

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

import group_cases as C  # noqa: E402

DEV = "cuda:0"
DTS = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def to_dev(bits, dt):
    a = np.ascontiguousarray(bits)
    return torch.from_numpy(a.view(np.int32 if dt == "fp32" else np.int16)).view(DTS[dt]).to(DEV)


def from_dev(t, dt):
    """-> bit patterns (uint16 / uint32) of a tensor"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if dt == "fp32" else torch.int16).numpy().view(C.uint_of(dt))


def report(got, want, dt, what):
    d = C.differs(got, want, dt)
    if not d.any():
        return None
    idx = np.argwhere(d)
    return f"{what}: {len(idx)} of {d.size} differ, first at {idx[:4].tolist()} got {[hex(int(got[tuple(i)])) for i in idx[:4]]} want {[hex(int(want[tuple(i)])) for i in idx[:4]]}"


def run_cross(dt, kind, nbits=4, rowwise=True):
    """every case of case_list(dt) through fq_group_fwd under cpu_eager: one kernel launch each (counted), every element against the
    oracle on the [rows * cols / g, g] view and (rowwise) against the row-wise kernels on the same view -> (cases run, failure texts)"""
    import llm_qat_amd
    from llm_qat_amd import ops
    llm_qat_amd.set_semantics("cpu_eager")
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    cases = C.case_list(dt)
    for c in cases:
        x = to_dev(C.cached_inputs(dt, c), dt)
        before = dict(ops.group_counts)
        y = fn(x, nbits, group_size=c.g)
        after = dict(ops.group_counts)
        if after["group_launch"] != before["group_launch"] + 1 or after["group_view_route"] != before["group_view_route"]:
            failures.append(f"{c}: not served by the group kernel ({before} -> {after})")
            continue
        got = from_dev(y, dt)
        msg = report(got, C.cached_reference(dt, c, kind, nbits), dt, f"{dt} {kind} {c} vs the oracle")
        if msg:
            failures.append(msg)
        if rowwise:
            msg = report(got, from_dev(fn(x.reshape(-1, c.g), nbits).reshape(x.shape), dt), dt, f"{dt} {kind} {c} vs the row-wise kernels")
            if msg:
                failures.append(msg)
    return len(cases), failures


def main(out):
    assert os.environ.get("LLMQAT_FQ_NT_LOAD_MIN_MB") == "0", "start this worker with LLMQAT_FQ_NT_LOAD_MIN_MB=0"
    total, failures = 0, []
    for dt in ("bf16", "fp32"):
        for kind in ("sym", "asym"):
            n, f = run_cross(dt, kind, rowwise=False)
            total += n
            failures += f
    torch.cuda.synchronize()
    with open(out, "w") as fh:
        json.dump({"cases": total, "failures": failures[:20]}, fh)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
