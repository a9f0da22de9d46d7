#!/usr/bin/env python3
"""Per-launch figures of the headline step from rocprofv3 runs of a plain `bench.py` (no extras, no sustained leg).

    python tools/step_trace_summary.py <trace_dir> [<fetch_dir> <write_dir>] [--json OUT]

<trace_dir>: `rocprofv3 --kernel-trace --output-format csv -d <trace_dir> -- python bench.py ...`; the two PMC directories are
the same command with `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate runs).  The step's launches are the fq:: dispatches at
the step's grid (the pair forward: one workgroup per row of both tensors; the pair backward: the same rows, 256 threads);
dispatches of other shapes (set-up, checks) are left out.  For each launch kind: median / mean duration, and, with the PMC
runs, the median HBM bytes (FETCH_SIZE doubled for 16-byte-per-lane streams, WRITE_SIZE as is: profiles/README.md) and the
byte rate over the median duration.  The step gap is the median time from a forward's start to the next forward's start
minus the two launches: what the same-stream boundaries and the host add per step.
"""
import csv
import glob
import json
import os
import statistics
import sys

ROLES = (("fq_sym_fwd_pair", "row_reg_kernel"), ("fq_ste_bwd_mask_pair", "ste_mask_kernel"))


def _rows(d, pattern):
    files = glob.glob(os.path.join(d, "**", pattern), recursive=True)
    if not files:
        raise SystemExit(f"no {pattern} under {d}")
    out = []
    for f in files:
        with open(f, newline="") as fh:
            out.extend(csv.DictReader(fh))
    return out


def _grid(r):
    if "Grid_Size_X" in r:
        return int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"])
    return int(r["Grid_Size"])


def _step_dispatches(rows):
    """{role: [row, ...]} for the step's two kernels at their most frequent grid (the timed loop dominates the counts)."""
    out = {}
    for role, kern in ROLES:
        mine = [r for r in rows if kern in r["Kernel_Name"] and "fq::" in r["Kernel_Name"]]
        if not mine:
            raise SystemExit(f"no {kern} dispatch")
        grids = [_grid(r) for r in mine]
        g = max(set(grids), key=grids.count)
        out[role] = sorted((r for r in mine if _grid(r) == g), key=lambda r: int(r["Dispatch_Id"]))
    return out


def summarize(trace_dir, fetch_dir=None, write_dir=None):
    tr = _step_dispatches(_rows(trace_dir, "*kernel_trace.csv"))
    res = {}
    for role, rs in tr.items():
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs]
        res[role] = {"kernel": rs[0]["Kernel_Name"].split("(")[0], "launches": len(d), "median_us": round(statistics.median(d), 2),
                     "mean_us": round(statistics.mean(d), 2)}
    fw, bw = tr[ROLES[0][0]], tr[ROLES[1][0]]
    starts = [int(r["Start_Timestamp"]) for r in fw]
    periods = [(b - a) / 1e3 for a, b in zip(starts, starts[1:])]
    period = statistics.median(periods)
    res["step_period_us"] = round(period, 2)
    res["step_gap_us"] = round(period - res[ROLES[0][0]]["median_us"] - res[ROLES[1][0]]["median_us"], 2)
    for tag, d, scale in (("fetch", fetch_dir, 2.0), ("write", write_dir, 1.0)):
        if not d:
            continue
        pm = _step_dispatches(_rows(d, "*counter_collection.csv"))
        for role, rs in pm.items():
            res[role][f"{tag}_mb"] = round(statistics.median(float(r["Counter_Value"]) for r in rs) * 1024 * scale / 1e6, 1)
    for role, _ in ROLES:
        e = res[role]
        if "fetch_mb" in e and "write_mb" in e:
            e["hbm_mb"] = round(e["fetch_mb"] + e["write_mb"], 1)
            e["tb_s"] = round(e["hbm_mb"] * 1e6 / (e["median_us"] * 1e-6) / 1e12, 2)
    return res


def main(argv):
    js = None
    if "--json" in argv:
        i = argv.index("--json")
        js = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if len(argv) not in (1, 3):
        raise SystemExit(__doc__)
    res = summarize(*argv)
    text = json.dumps(res, indent=1)
    print(text)
    if js:
        with open(js, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
