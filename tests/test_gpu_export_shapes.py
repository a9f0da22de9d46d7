"""GPU tier of the export kernels at every launch shape, row mode and container (tests/export_cases.py; the CPU tier
tests/test_export_cases_cpu.py proves that these inputs expose a wrong rounding, clamp, count or packing).  Zero tolerance: every packed
byte, every scale as bits, every overflow count against the CPU oracle (`export_cases.expected`), under cpu_eager.  The one relaxation is the
one tests/test_gpu_export.py has: Asym beta may differ in the sign of zero.

The cross: 2808 launches over the 18 rungs of by_reg_shape (fq_shapes.h), which launch_export_reg follows (bf16 1188, fp16 900,
fp32 720), plus a device_eager slice; dequantisation of the clean rows; the generic kernel on the same adversarial rows (odd widths, rows beyond the register kernels, element-aligned
storage); the scale pre-pass with bounds and bitmap through the C ABI; canaries around bins, scales and overflow; the non-temporal load
instantiation in a child interpreter.  Nothing is skipped: a combination a dtype cannot hold is absent from export_cases.COMBOS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import export_cases as E
import export_ntl_worker as W
import group_cases as C
from conftest import ROOT
from export_cases import EPV, RUNGS
from group_ntl_worker import DEV, DTS, from_dev, to_dev
from row_ntl_worker import unpack_mask
from row_view_cases import row_bits

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "fp16", "fp32"]
KINDS = ["sym", "asym"]


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


def tail_shapes(dt):
    return [sh for sh in E.widths(dt) if sh.kind == "tail" and sh.rows == 5]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_cross(dt, kind):
    cases = E.cross(dt, kind)
    n, failures = W.run_cases(dt, cases)
    assert n == len(cases) >= 18 * 2 * 4
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt", DTYPES)
def test_device_eager_at_every_rungs_tail_width(dt):
    import llm_qat_amd
    llm_qat_amd.set_semantics("device_eager")
    cases = [(c, sh) for sh in tail_shapes(dt) for c in (E.Combo("sym", 8, "int8", False), E.Combo("asym", 8, "int8", False))]
    n, failures = W.run_cases(dt, cases, sem=1)
    assert n == 2 * len(RUNGS)
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt", DTYPES)
def test_dequantised_clean_rows_equal_the_forward(dt):
    """where a case's expected overflow row is 0, dequantize() == the fake-quant forward of that row bit for bit, up to the sign of zero:
    every 5-row shape x every combination outside autocast (whose forward returns fp32 and is not what dequantize() restates) up to 16
    bits (the widths the forward kernels are tested at)"""
    from llm_qat_amd import ops
    cases = 0
    for sh in E.widths(dt):
        if sh.rows != 5:
            continue
        for c in E.combos(dt, autocast=False):
            if c.bits > 16:
                continue
            clean = torch.from_numpy(E.expected(dt, *c, sh.cols, sh.rows)[2] == 0)
            if dt != "fp16":
                assert int(clean.sum()) >= 2, (dt, c, sh)          # the tiny row and the row of zeros at the least
            if not clean.any():
                continue
            x = to_dev(E.export_inputs(dt, *c, sh.cols, sh.rows), dt)
            d = W.export(x, c).dequantize()
            y = ops.sym_quantize(x, c.bits) if c.kind == "sym" else ops.asym_quantize(x, c.bits)
            d, y = d[clean.to(DEV)], y[clean.to(DEV)]
            z = torch.zeros_like(d)
            assert torch.equal(torch.where(d == 0, z, d), torch.where(y == 0, z, y)), (dt, c, sh)
            cases += 1
    n = 2 * len(RUNGS) * len([c for c in E.combos(dt, autocast=False) if c.bits <= 16])
    assert cases == n if dt != "fp16" else cases >= n // 3, (cases, n)     # (fp16 has no mode-0 row at a saturating width: see export_cases)


GENERIC_COMBOS = [E.Combo("sym", 4, "int4", False), E.Combo("sym", 8, "int4", False), E.Combo("sym", 16, "int8", False), E.Combo("sym", 17, "int16", False),
                  E.Combo("asym", 4, "int4", False), E.Combo("asym", 8, "int4", False), E.Combo("asym", 16, "int8", False), E.Combo("asym", 17, "int16", False),
                  E.Combo("sym", 4, "int4", True), E.Combo("sym", 16, "int8", True), E.Combo("sym", 8, "int16", True)]


def generic_widths(dt):
    epv = EPV[dt]
    return [1, 2, epv - 1, epv + 1, 255, 257, 511, 513, 1023, E.REG_MAX_VEC * epv + 1, (E.REG_MAX_VEC + 1) * epv]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
def test_generic_kernel_on_the_same_rows(dt, rows):
    """row_export_generic_kernel: widths that are no multiple of a vector, one odd and one even width beyond the register kernels, and
    (every width) storage that is only element-aligned"""
    epv = EPV[dt]
    failures = []
    n = 0
    for cols in generic_widths(dt):
        for c in GENERIC_COMBOS:
            if c.autocast and dt == "fp32":
                continue
            bits = E.export_inputs(dt, *c, cols, rows)
            want = E.expected(dt, *c, cols, rows)
            x = to_dev(bits, dt)
            flat = torch.empty(rows * cols + 1, dtype=DTS[dt], device=DEV)
            flat[1:].copy_(x.reshape(-1))
            for how, xin in (("aligned", x), ("element-aligned", flat[1:].view(rows, cols))):
                if how == "aligned" and cols % epv == 0 and cols // epv <= E.REG_MAX_VEC:
                    continue                                            # (the register kernels' business)
                assert how == "aligned" or xin.data_ptr() % 16
                e = W.export(xin, c)
                got = W.raw_bytes(e, rows)
                n += 1
                msg = W.compare(got, e.scales.cpu().numpy(), e.overflow.cpu().numpy(), want, c, f"{dt} {c} [{rows}, {cols}] {how}")
                if msg:
                    failures.append(msg)
                if c.container == "int4" and cols % 2:
                    assert (got[:, -1] >> 4 == 0).all(), (dt, c, cols, how, "the unused high nibble of an odd row's last byte")
    assert n >= 2 * 9 * 8
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("dt,autocast", [("bf16", False), ("bf16", True), ("fp32", False)])
def test_scale_prepass_with_bounds_and_bitmap_at_every_rung(dt, autocast):
    """fq_sym_row_scales with row_bounds_out and mask_out (container = NONE, the general body's mask path): scales == the oracle, bounds ==
    the rows' max / -max of |x|, bitmap rows of clippable rows == the clip predicate, the other rows of the bitmap left as they were"""
    from llm_qat_amd import _lib, ops
    from oracle import oracle as O
    L = _lib.lib()
    code = ops._DTYPES[DTS[dt]]
    sem = 1 if autocast else 0
    shapes = [sh for sh in E.widths(dt) if sh.rows == 5]
    assert len(shapes) == 2 * len(RUNGS)
    for sh in shapes:
        rows, cols = sh.rows, sh.cols
        b = row_bits(dt, cols, rows)
        x = to_dev(b, dt)
        mb = L.fq_ste_mask_bytes(rows, cols, code)
        assert mb == rows * ((cols + 63) // 64) * 8
        mask = torch.full((mb,), 0xA5, dtype=torch.uint8, device=DEV)
        bounds = torch.full((rows, 2), 7.0, device=DEV)
        scales = torch.full((rows, 2), 7.0, device=DEV)
        rc = L.fq_sym_row_scales(x.data_ptr(), scales.data_ptr(), rows, cols, 8, code, sem, 1 if autocast else 0, -2.0, 2.0, bounds.data_ptr(),
                                 mask.data_ptr(), mb, ops._stream(x))
        assert rc == 0, L.fq_last_error()
        torch.cuda.synchronize()
        want_sc = O.export("sym", C.oracle_view(b, dt), rows, cols, 8, "int8", dt, sem=sem, autocast=autocast)[1]
        assert E.scales_equal(scales.cpu().numpy(), want_sc, False), (dt, sh)
        want_b = C.row_bounds(b, dt, False)
        assert not C.differs(from_dev(bounds, "fp32"), want_b.view(np.uint32), "fp32").any(), (dt, sh)
        clippable = ~((want_b[:, 0] < 2.0) & (want_b[:, 1] > -2.0))
        assert clippable.any() and (~clippable).any()
        mbits, mraw = unpack_mask(mask, rows, cols), mask.cpu().numpy().reshape(rows, -1)
        assert np.array_equal(mbits[clippable], C.clip_predicate(b, dt)[clippable]), (dt, sh)
        assert (mraw[~clippable] == 0xA5).all(), (dt, sh, "a row that cannot clip had its bitmap row written")


@pytest.mark.parametrize("dt", DTYPES)
def test_canaries_around_bins_scales_and_overflow(dt):
    """the raw C ABI at every rung's tail width, int4 and int8: nothing is written outside bins, scales and overflow"""
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    code = ops._DTYPES[DTS[dt]]
    conts = {"int4": _lib.BINS_INT4, "int8": _lib.BINS_INT8}
    pad = 4096
    for sh in tail_shapes(dt):
        rows, cols = sh.rows, sh.cols
        for c in (E.Combo("sym", 8, "int4", False), E.Combo("sym", 16, "int8", False), E.Combo("asym", 8, "int4", False), E.Combo("asym", 16, "int8", False)):
            x = to_dev(E.export_inputs(dt, *c, cols, rows), dt)
            nb = L.fq_export_bins_bytes(rows, cols, conts[c.container])
            bbuf = torch.full((nb + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
            sbuf = torch.full((2 * rows + 2 * pad,), 3.0, device=DEV)
            obuf = torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=DEV)
            head = (x.data_ptr(), bbuf[pad:].data_ptr(), sbuf[pad:].data_ptr(), obuf[pad:].data_ptr(), rows, cols, c.bits, conts[c.container], code, 0)
            rc = L.fq_sym_export(*head, 0, ops._stream(x)) if c.kind == "sym" else L.fq_asym_export(*head, ops._stream(x))
            assert rc == 0, L.fq_last_error()
            torch.cuda.synchronize()
            assert (bbuf[:pad] == 0xA5).all() and (bbuf[pad + nb:] == 0xA5).all(), (dt, c, sh)
            assert (sbuf[:pad] == 3.0).all() and (sbuf[pad + 2 * rows:] == 3.0).all(), (dt, c, sh)
            assert (obuf[:pad] == -77).all() and (obuf[pad + rows:] == -77).all(), (dt, c, sh)
            msg = W.compare(bbuf[pad:pad + nb].view(rows, -1).cpu().numpy(), sbuf[pad:pad + 2 * rows].view(rows, 2).cpu().numpy(),
                            obuf[pad:pad + rows].cpu().numpy(), E.expected(dt, *c, cols, rows), c, f"{dt} {c} {sh}")
            assert msg is None, msg


def test_non_temporal_load_instantiation_in_a_fresh_interpreter(tmp_path):
    """LLMQAT_FQ_NT_LOAD_MIN_MB is read once per process: a child interpreter with it set to 0 runs every 5-row shape (bf16 and fp32, Sym
    and Asym, a fitting and a saturating combination per container) with every load non-temporal, against the oracle"""
    torch.cuda.synchronize()      # (nothing is started next to a device that has already reported an error)
    out = str(tmp_path / "ntl.json")
    env = dict(os.environ, LLMQAT_FQ_NT_LOAD_MIN_MB="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "export_ntl_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert os.path.exists(out), (p.returncode, p.stderr[-1500:])
    with open(out) as fh:
        doc = json.load(fh)
    assert p.returncode == 0 and not doc["failures"], (p.returncode, doc["failures"][:5], p.stderr[-1500:])
    assert doc["cases"] == sum(len(W.ntl_cases(dt)) for dt in W.NTL_DTYPES) == 2 * 36 * 12
