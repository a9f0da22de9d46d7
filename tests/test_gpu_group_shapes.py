"""GPU tier of the group-wise kernel at every launch shape, group width and row tail (tests/group_cases.py; the CPU tier
tests/test_group_cases_cpu.py proves that these inputs expose a wrong reduction).  Zero tolerance on bits, any NaN equals any NaN, every
element compared.  The reference is the CPU oracle on the [rows * cols / g, g] view, which shares nothing with the kernels; the row-wise
kernels on the same view are a second check.  Every case asserts that fq_group_fwd served it (one launch, no view route).

Plain mode: the whole case list at 4 bits (Sym / Asym x bf16 / fp16 / fp32), the tail rows at 3, 4, 8 and 16 bits under both arithmetic
policies, the autocast arithmetic on 16-bit tensors.  Training mode: y, the full-row bounds, the bitmap of clippable rows (against the
predicate and against the row-wise training forward), the unchanged STE backward on it, canaries around every output.  The non-temporal
load branch: the 4-bit cross once more in a child interpreter that forces it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import group_cases as C
import group_ntl_worker as W
from conftest import ROOT
from group_cases import BRACKETS, GVS
from group_ntl_worker import DEV, DTS, from_dev, report, to_dev

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "fp16", "fp32"]
KINDS = ["sym", "asym"]
SEMS = {"cpu_eager": 0, "device_eager": 1}


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    yield
    llm_qat_amd.set_semantics(prev)


def served(before):
    """fq_group_fwd ran exactly once since `before` and nothing took the view route"""
    from llm_qat_amd import ops
    now = ops.group_counts
    return now["group_launch"] == before["group_launch"] + 1 and now["group_view_route"] == before["group_view_route"]


def counts():
    from llm_qat_amd import ops
    return dict(ops.group_counts)


def tail_cases(dt, gvs):
    """per bracket and gv the tail row (the full row where the bracket holds one multiple of gv only), 5 rows"""
    cases = [c for c in C.case_list(dt) if c.rows == 5 and c.gv in gvs]
    out = []
    for bi in range(len(BRACKETS)):
        for gv in gvs:
            mine = {c.kind: c for c in cases if c.bracket == bi and c.gv == gv}
            out.append(mine.get("tail", mine["full"]))
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_full_cross_at_four_bits(dt, kind):
    n, failures = W.run_cross(dt, kind, 4, rowwise=True)
    assert n >= 3 * 10 * len(GVS) - 12           # three row lengths per bracket and gv, less the brackets that hold fewer multiples of gv
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_tail_rows_at_other_widths_and_both_semantics(dt, kind):
    """bits 3 / 4 / 8 / 16 (bf16 Asym: both sides of the reciprocal-multiply switch at 8 bits) under cpu_eager and device_eager"""
    import llm_qat_amd
    from llm_qat_amd import ops
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    for c in tail_cases(dt, (4, 64)):
        x = to_dev(C.cached_inputs(dt, c), dt)
        for sem, code in SEMS.items():
            llm_qat_amd.set_semantics(sem)
            for nbits in (3, 4, 8, 16):
                before = counts()
                y = fn(x, nbits, group_size=c.g)
                assert served(before), c
                got = from_dev(y, dt)
                failures.append(report(got, C.cached_reference(dt, c, kind, nbits, code), dt, f"{c} {sem} bits {nbits} vs the oracle"))
                failures.append(report(got, from_dev(fn(x.reshape(-1, c.g), nbits).reshape(x.shape), dt), dt,
                                       f"{c} {sem} bits {nbits} vs the row-wise kernels"))
    failures = [f for f in failures if f]
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_arithmetic_at_every_bracket_and_width(dt):
    from llm_qat_amd import ops
    failures = []
    for c in tail_cases(dt, GVS):
        x = to_dev(C.cached_inputs(dt, c), dt)
        for nbits in (4, 8):
            before = counts()
            res = ops.group_forward("sym", x, nbits, c.g, autocast=True)
            assert res is not None and served(before), c
            failures.append(report(from_dev(res[0], dt), C.cached_reference(dt, c, "sym", nbits, autocast=True), dt, f"{c} autocast bits {nbits}"))
    failures = [f for f in failures if f]
    assert not failures, (len(failures), failures[:5])


def unpack_mask(mask, rows, cols):
    """the row bitmap (rows padded to 8 bytes) -> bool [rows, cols]"""
    m = mask.cpu().numpy().reshape(rows, -1)
    assert m.shape[1] == (cols + 63) // 64 * 8
    return np.unpackbits(m, axis=1, bitorder="little")[:, :cols].astype(bool)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_training_mode_at_every_bracket(dt, kind):
    from llm_qat_amd import ops
    from oracle import oracle as O
    import llm_qat_amd
    llm_qat_amd.set_semantics("cpu_eager")
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    for c in C.train_cases(dt):
        bits = C.cached_inputs(dt, c, train=True)
        x = to_dev(bits, dt)
        before = counts()
        res = ops.quantize_train(kind, x, 4, False, -2.0, 2.0, group_size=c.g)
        assert res is not None and served(before), c
        y, bounds, mask = res
        got = from_dev(y, dt)
        failures.append(report(got, from_dev(fn(x, 4, group_size=c.g), dt), dt, f"{c} y vs plain mode"))
        failures.append(report(got, C.cached_reference(dt, c, kind, 4, train=True), dt, f"{c} y vs the oracle"))
        # full-row bounds, from the bits
        want_b = C.row_bounds(bits, dt, kind == "asym")
        failures.append(report(from_dev(bounds, "fp32"), want_b.view(np.uint32), "fp32", f"{c} bounds"))
        clippable = ~((want_b[:, 0] < 2.0) & (want_b[:, 1] > -2.0))
        assert clippable.any() and (~clippable).any()
        pred = C.clip_predicate(bits, dt)
        mbits = unpack_mask(mask, c.rows, c.cols)
        if not np.array_equal(mbits[clippable], pred[clippable]):
            failures.append(f"{c} bitmap differs from the predicate at {np.argwhere(mbits[clippable] != pred[clippable])[:4].tolist()}")
        # what the row-wise training forward of the whole row writes
        rw = ops.quantize_train(kind, x, 4, False, -2.0, 2.0)
        assert rw is not None
        failures.append(report(from_dev(bounds, "fp32"), from_dev(rw[1], "fp32"), "fp32", f"{c} bounds vs the row-wise training forward"))
        if not np.array_equal(mbits[clippable], unpack_mask(rw[2], c.rows, c.cols)[clippable]):
            failures.append(f"{c} bitmap differs from the row-wise training forward's")
        # the unchanged backward on these side outputs: NaN, +-Inf and -0.0 in the gradient at zeroed and at kept positions
        gb = C.grad_bits(pred, dt, c.seed)
        want_g = O.ste_bwd(C.oracle_view(gb, dt), C.oracle_view(bits, dt), -2.0, 2.0, dt).view(C.uint_of(dt))
        gout = to_dev(gb, dt)
        failures.append(report(from_dev(ops.ste_backward_mask(gout, -2.0, 2.0, bounds, mask, c.rows, c.cols), dt), want_g, dt, f"{c} backward"))
        gin = gout.clone()
        out = ops.ste_backward_mask(gin, -2.0, 2.0, bounds, mask, c.rows, c.cols, inplace=True)
        assert out.data_ptr() == gin.data_ptr()
        failures.append(report(from_dev(out, dt), want_g, dt, f"{c} backward in place"))
    failures = [f for f in failures if f]
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt", DTYPES)
def test_training_mode_canaries_on_tail_rows(dt):
    """a tail row of a four-rows-per-workgroup shape and of a multi-wave shape, 5 rows: nothing is written outside y, the bounds, the mask"""
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    pad = 4096
    picked = [c for c in C.train_cases(dt) if c.rows == 5 and c.kind == "tail" and (c.bracket, c.gv) in ((1, 4), (6, 64))]
    assert len(picked) == 2
    for c in picked:
        bits = C.cached_inputs(dt, c, train=True)
        x = to_dev(bits, dt)
        n = c.rows * c.cols
        code = ops._DTYPES[x.dtype]
        for asym in (0, 1):
            ybuf = torch.full((n + 2 * pad,), 7.0, device=DEV, dtype=DTS[dt])
            mb = L.fq_ste_mask_bytes(c.rows, c.cols, code)
            mbuf = torch.full((mb + 2 * pad,), 0xA5, device=DEV, dtype=torch.uint8)
            bbuf = torch.full((c.rows * 2 + 2 * pad,), 3.0, device=DEV, dtype=torch.float32)
            y = ybuf[pad:pad + n]
            rc = L.fq_group_fwd(asym, x.data_ptr(), y.data_ptr(), c.rows, c.cols, c.g, 4, code, 0, 0, -2.0, 2.0, bbuf[pad:].data_ptr(),
                                mbuf[pad:].data_ptr(), mb, ops._stream(x))
            assert rc == 0, L.fq_last_error()
            torch.cuda.synchronize()
            assert (ybuf[:pad] == 7.0).all() and (ybuf[pad + n:] == 7.0).all()
            assert (mbuf[:pad] == 0xA5).all() and (mbuf[pad + mb:] == 0xA5).all()
            assert (bbuf[:pad] == 3.0).all() and (bbuf[pad + 2 * c.rows:] == 3.0).all()
            kind = "asym" if asym else "sym"
            assert report(from_dev(y.view(c.rows, c.cols), dt), C.cached_reference(dt, c, kind, 4, train=True), dt, f"{c} {kind}") is None


def test_non_temporal_load_branch_in_a_fresh_interpreter(tmp_path):
    """LLMQAT_FQ_NT_LOAD_MIN_MB is read once per process: a child interpreter with it set to 0 runs the 4-bit cross (bf16 and fp32, Sym
    and Asym) with every load non-temporal, against the oracle"""
    torch.cuda.synchronize()      # (nothing is started next to a device that has already reported an error)
    out = str(tmp_path / "ntl.json")
    env = dict(os.environ, LLMQAT_FQ_NT_LOAD_MIN_MB="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "group_ntl_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert os.path.exists(out), (p.returncode, p.stderr[-1500:])
    with open(out) as fh:
        doc = json.load(fh)
    assert p.returncode == 0 and not doc["failures"], (p.returncode, doc["failures"][:5], p.stderr[-1500:])
    assert doc["cases"] == 2 * (len(C.case_list("bf16")) + len(C.case_list("fp32")))
