"""Every launch shape the host dispatch of the row kernels can pick, on the MI355X: one width per rung of the register ladder (forward,
plain and training mode, Sym and Asym, and the autocast arithmetic), every half-vector count of the fp32-result forward, every vector count
of the mask backwards in each of their launch forms, and one case per (kind, rotate, ceil, mask) of the MX launcher.  The dispatch is
host code, so a wrong rung shows as a wrong result or not at all: zero tolerance on bits, any NaN equals any NaN, every element compared.
References: the CPU oracle (oracle/oracle.py) for the forwards, the clip predicate on x for the bitmaps and the backwards, the numpy MX
references of the MX tests.

A width is cols = (nvec - 1) * EPV for a rung whose rows hold up to nvec 16-byte vectors, so the last lane-slot of the row is the clamped
duplicate of the last vector; 5 rows, so the kernels that put four rows into a workgroup run a partly empty last one."""
import numpy as np
import pytest
import torch

import mx_rules_reference as R
import row_ntl_worker as W
from group_ntl_worker import report, to_dev
from mx_reference import pack_fp4
from mx_rot_reference import rotate_bits
from mx_rules_cases import rand_bits
# the inputs, the memoised references and the ladders live in row_view_cases.py, the loops in row_ntl_worker.py: this file, the pitched
# walk, the multi-tensor walk and the non-temporal-load worker use one copy (RUNGS and NVECS: tests/test_shape_tables_cpu.py reads them here)
from row_ntl_worker import none_failed
from row_view_cases import NVECS, RUNGS, backward_vpt  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


# ---- forward: every rung of the register ladder ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_forward_plain_and_training_at_every_rung(dt, kind):
    none_failed(W.forward_plain_and_training(dt, kind))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_narrow_at_every_rung(dt):
    none_failed(W.autocast_narrow(dt))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_wide_at_every_half_vector_count(dt):
    none_failed(W.autocast_wide(dt))


# ---- backward from (bounds, bitmap): every vector count in every launch form ---------------------------------------------------------------

def test_the_rung_widths_reach_every_backward_vector_count():
    assert {backward_vpt(n - 1) for n in NVECS} == set(range(1, 9))


@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_mask_backward_one_tensor_and_in_place(dt, kind):
    none_failed(W.mask_backward_one_tensor_and_in_place(dt, kind))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_mask_backward_two_and_four_slot_forms(dt):
    """the two-slot form (pair_backward: both copying, and the first slot in place as a weight's gradient is) and the four-slot form
    (multi_backward with three tensors, the first in place): tensors of 5, 3 and 4 rows of the same width"""
    none_failed(W.mask_backward_two_and_four_slot_forms(dt))


def test_non_temporal_loads_in_a_fresh_interpreter(tmp_path):
    """LLMQAT_FQ_NT_LOAD_MIN_MB is read once per process: ONE child interpreter with it set to 0 runs the loops above, the x-reading and
    flat backwards and the multi-tensor forward once more (tests/row_ntl_worker.py walk(): bf16, and fp32 where the form serves it), so
    that every launch takes its streamed instantiation"""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    torch.cuda.synchronize()      # (nothing is started next to a device that has already reported an error)
    out = str(tmp_path / "row_ntl.json")
    env = dict(os.environ, LLMQAT_FQ_NT_LOAD_MIN_MB="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "row_ntl_worker.py"), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert os.path.exists(out), (p.returncode, p.stderr[-1500:])
    with open(out) as fh:
        doc = json.load(fh)
    assert p.returncode == 0 and not doc["failures"], (p.returncode, doc["failures"][:5], p.stderr[-1500:])
    assert doc["cases"] == W.walk_launches()


# ---- MX: one case per combination the one launcher serves ----------------------------------------------------------------------------------

MX_SHAPE = (64, 128)


def bits16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("rule", ["floor", "ceil"])
@pytest.mark.parametrize("rotate", [False, True])
def test_mx_forward_mask_and_exports(rotate, rule):
    from llm_qat_amd import ops
    b = rand_bits(MX_SHAPE, "bf16", 77)
    x = to_dev(b, "bf16")
    want = R.quantize_bits(b, "bf16", "mxfp4", rule, rotate).reshape(MX_SHAPE)
    assert report(bits16(ops.mx_quantize(x, "mxfp4", rotate=rotate, scale_rule=rule)), want, "bf16", "forward") is None
    y, mask = ops.mx_quantize(x, "mxfp4", rotate=rotate, scale_rule=rule, return_mask=True)
    assert report(bits16(y), want, "bf16", "forward with the bitmap") is None
    assert np.array_equal(mask.cpu().numpy(), R.pack_mask(R.keep_mask(b, "bf16", "mxfp4", rule, rotate)))
    for fmt in ("mxfp4", "mxfp8_e4m3"):
        e = ops.mx_export(x, fmt, rotate=rotate, scale_rule=rule)
        codes, scales = R.export_bits(b, "bf16", fmt, rule, rotate)
        assert np.array_equal(e.scales.cpu().numpy().reshape(-1), scales), fmt
        assert np.array_equal(e.elements.cpu().numpy().reshape(-1), pack_fp4(codes) if fmt == "mxfp4" else codes), fmt


def test_mx_rotation_alone():
    from llm_qat_amd import ops
    b = rand_bits(MX_SHAPE, "bf16", 78)
    assert report(bits16(ops.mx_rotate(to_dev(b, "bf16"))), rotate_bits(b, "bf16").reshape(MX_SHAPE), "bf16", "rotation") is None
