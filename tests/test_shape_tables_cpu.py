"""CPU tier: the one place where the launch-shape tables of the C++ launch layer (llm-qat_amd/csrc/fq_shapes.h: by_reg_shape, by_group_shape,
by_count) meet their Python mirrors in the tests (export_cases.RUNGS, test_gpu_row_launch_shapes.RUNGS, group_cases.BRACKETS).
tests/c_host/shape_tables.cpp includes fq_shapes.h alone and prints what the tables give for every nvec in 1 .. 8192; the mirrors must
say the same for every one of them.  No kernel runs and no HIP header is read."""
import os
import subprocess

import pytest

import export_cases as E
import group_cases as G
from conftest import ROOT

REG_MAX_VEC = 8192


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """-> {"reg": {nvec: (tpr, vpt)}, "group": {nvec: (tpr, vpt)}, "count": {n: served}} as the compiled header gives them"""
    exe = str(tmp_path_factory.mktemp("shape_tables") / "shape_tables")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "llm-qat_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "c_host", "shape_tables.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    t = {"reg": {}, "group": {}, "count": {}}
    for line in out.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        assert v[0] not in t[kind], line            # one shape per nvec
        t[kind][v[0]] = v[1] if kind == "count" else (v[1], v[2])
    return t


def test_the_program_reads_the_header_alone():
    src = open(os.path.join(ROOT, "tests", "c_host", "shape_tables.cpp")).read()
    assert [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")] == ["<cstdio>", '"fq_shapes.h"']
    hdr = open(os.path.join(ROOT, "llm-qat_amd", "csrc", "fq_shapes.h")).read()
    assert sorted(ln.split()[1] for ln in hdr.splitlines() if ln.startswith("#include")) == ["<cstdint>", "<type_traits>"]


def test_every_nvec_has_a_shape_that_holds_it(tables):
    for kind in ("reg", "group"):
        assert sorted(tables[kind]) == list(range(1, REG_MAX_VEC + 1))
        for nvec, (tpr, vpt) in tables[kind].items():
            assert tpr * vpt >= nvec, (kind, nvec, tpr, vpt)
            assert tpr in (64, 128, 256, 512, 1024) and 1 <= vpt <= 8, (kind, nvec, tpr, vpt)
    for nvec, (tpr, vpt) in tables["group"].items():        # whole groups of up to 64 vectors in every rung
        assert tpr * vpt % 64 == 0, (nvec, tpr, vpt)
    assert tables["count"] == {n: int(1 <= n <= 8) for n in range(10)}


def test_export_cases_rungs_equal_by_reg_shape(tables):
    assert E.REG_MAX_VEC == REG_MAX_VEC
    for nvec in range(1, REG_MAX_VEC + 1):
        r = E.RUNGS[E.rung_of(nvec)]
        assert (r.tpr, r.slots) == tables["reg"][nvec], (nvec, r)


def test_row_launch_shapes_rungs_equal_by_reg_shape(tables):
    """test_gpu_row_launch_shapes.RUNGS: threads per row -> the largest nvec of each of its rungs (one rung per vectors-per-thread count
    the row needs; 5 and 7 run the 6- and 8-slot kernels)"""
    import test_gpu_row_launch_shapes as S
    tops = sorted((top, tpr) for tpr, ts in S.RUNGS.items() for top in ts)
    assert tops[-1][0] == REG_MAX_VEC and len(tops) == 18
    lo = 0
    for top, tpr in tops:
        need = -(-top // tpr)
        for nvec in range(lo + 1, top + 1):
            assert tables["reg"][nvec] == (tpr, {5: 6, 7: 8}.get(need, need)), (nvec, tpr, top)
        lo = top
    assert S.NVECS == [top for tpr in S.RUNGS for top in S.RUNGS[tpr]]


def test_group_cases_brackets_equal_by_group_shape(tables):
    assert G.BRACKETS[0].lo == 0 and G.BRACKETS[-1].hi == REG_MAX_VEC
    for nvec in range(1, REG_MAX_VEC + 1):
        b = G.BRACKETS[G.bracket_of(nvec)]
        assert (b.tpr, b.vpt) == tables["group"][nvec], (nvec, b)
