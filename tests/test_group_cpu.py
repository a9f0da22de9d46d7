"""CPU tier of group-wise fake quantization (one scale per `group_size` consecutive elements of a row): argument checks of the Python
API and of fq_group_fwd (no launch), the oracle on reshaped views against tests/golden/group.npz, the grouped export's dequantize() on CPU
tensors, and -- with the opt-in CPU-tensor path -- QuantizeLinear with group sizes against the reference's classes on the view."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

REF = os.environ.get("LLMQAT_REFERENCE", "/root/reference")


def load_group():
    z = np.load(os.path.join(GOLDEN, "group.npz"))
    return z, json.loads(str(z["manifest"]))["cases"]


def same(a, b, dtype):
    """bit equality with any NaN equal to any NaN (the fixtures' payloads are the CPU's)"""
    u = np.uint32 if dtype == "fp32" else np.uint16
    a, b = np.asarray(a).view(u).ravel(), np.asarray(b).view(u).ravel()
    e, m = (0x7F800000, 0x7FFFFF) if dtype == "fp32" else (0x7F80, 0x7F) if dtype == "bf16" else (0x7C00, 0x3FF)
    nan = lambda v: ((v & e) == e) & ((v & m) != 0)  # noqa: E731
    return bool(((a == b) | (nan(a) & nan(b))).all())


def test_group_size_argument_errors():
    import llm_qat_amd
    from llm_qat_amd import ops
    x = torch.zeros(4, 256)
    for bad in (0, -128, 96 + 1, 3.5, "128", True):
        with pytest.raises(ValueError):
            ops.check_group(tuple(x.shape), bad)
    assert ops.check_group((4, 256), 128) == 128 and ops.check_group((2, 3, 256), 256.0) == 256
    with pytest.raises(ValueError):
        ops.check_group((2, 2, 2, 256), 128)           # 4-D
    with pytest.raises(ValueError):
        ops.check_group((4, 256), 128, layerwise=True)
    # the public entry points check before touching a device
    with pytest.raises(ValueError):
        ops.sym_quantize(x, 4, group_size=100)
    with pytest.raises(ValueError):
        ops.asym_quantize(x, 4, group_size=0)
    with pytest.raises(ValueError):
        ops.quantize_train("sym", x, 4, True, -2.0, 2.0, group_size=128)
    with pytest.raises(ValueError):
        ops.sym_export(x, 4, group_size=-1)
    with pytest.raises(ValueError):
        ops.asym_export(x, 4, layerwise=True, group_size=128)
    with pytest.raises(ValueError):
        llm_qat_amd.group_quantize(x, torch.tensor([-2.0, 2.0]), 4, 96)
    with pytest.raises(ValueError):
        llm_qat_amd.group_quantize(torch.zeros(2, 2, 2, 256), torch.tensor([-2.0, 2.0]), 4, 128)
    Q = llm_qat_amd.QuantizeLinear
    with pytest.raises(ValueError):
        Q(300, 64, w_bits=4, a_bits=8, weight_group_size=128)      # does not divide in_features
    with pytest.raises(ValueError):
        Q(256, 64, w_bits=4, a_bits=8, act_group_size=96)
    with pytest.raises(ValueError):
        Q(256, 64, w_bits=4, a_bits=8, weight_group_size=128, weight_layerwise=True)
    with pytest.raises(ValueError):
        Q(256, 64, w_bits=2, a_bits=8, weight_group_size=128)      # the 1-/2-bit branches have no groups
    with pytest.raises(ValueError):
        Q(256, 64, w_bits=4, a_bits=32, act_group_size=128)


def test_quantize_linear_group_attributes_and_defaults():
    import llm_qat_amd
    m = llm_qat_amd.QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_group_size=128, act_group_size=64)
    assert (m.weight_group_size, m.act_group_size) == (128, 64)
    assert list(m.state_dict().keys()) == ["weight"]
    assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=4, a_bits=8).weight_group_size is None
    prev = llm_qat_amd.default_group_sizes(weight=128)
    try:
        assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=4, a_bits=8).weight_group_size == 128
        assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=4, a_bits=8, weight_group_size=64).weight_group_size == 64   # explicit wins
        assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=16, a_bits=16).act_group_size is None
        assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=32, a_bits=32).weight_group_size is None   # not quantized: no group
        with pytest.raises(ValueError):
            llm_qat_amd.default_group_sizes(act=0)
    finally:
        llm_qat_amd.default_group_sizes(*prev)
    assert llm_qat_amd.QuantizeLinear(256, 64, w_bits=4, a_bits=8).weight_group_size is None


def test_fq_group_fwd_validation_without_gpu():
    import ctypes
    from llm_qat_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(asym=0, x=p, y=p + 1024, rows=2, cols=256, group=128, bits=4, dtype=1, sem=0, ac=0, b=None, m=None, mb=0):
        return L.fq_group_fwd(asym, x, y, rows, cols, group, bits, dtype, sem, ac, -2.0, 2.0, b, m, mb, None)

    assert call(dtype=7) == -1
    assert call(asym=2) == -7
    assert call(bits=0) == -2 and call(bits=32) == -2
    assert call(sem=3) == -7
    assert call(ac=2) == -7
    assert call(ac=1, asym=1) == -1 and call(ac=1, dtype=0) == -1
    assert call(rows=-1) == -3
    for g in (0, -1, -(2 ** 63)):
        assert call(group=g) == -7
    assert call(group=2 ** 62) == -3 and call(group=96) == -3
    assert call(rows=2 ** 62, cols=2 ** 10) == -3          # rows * cols overflows
    assert call(rows=0) == 0 and call(cols=0) == 0
    assert call(x=None) == -4 and call(y=None) == -4
    assert call(y=p) == -7                                 # in place
    assert call(m=p + 2048) == -4                          # a mask needs the bounds
    assert call(dtype=3) == -8                             # float64: the view route
    assert call(group=16) == -8 and call(group=1024, cols=1024, dtype=2) == -8 and call(group=8, dtype=0) == -8   # group outside 4..64 vectors
    assert call(cols=8 * 8192 * 2, group=256) == -8        # row longer than the register kernels hold
    assert call(x=p + 2) == -8                             # misaligned
    assert call(b=p + 2048, m=p + 2560, mb=8) == -5         # mask buffer too small
    assert L.fq_last_error() != b""


def test_oracle_on_views_equals_group_fixture():
    """the CPU oracle (the row-wise op chain restated in C) on the [rows * C / g, g] view reproduces the reference's group results"""
    from oracle import oracle as O
    z, cases = load_group()
    assert len(cases) == 72
    for c in cases:
        x, y = z[c["name"] + "_x"], z[c["name"] + "_y"]
        rows, g = x.size // c["group"], c["group"]
        fn = O.sym_fwd if c["kind"] == "sym" else O.asym_fwd
        yo = fn(x.reshape(rows, g), rows, g, c["bits"], c["dtype"], want_idx=False)[0]
        assert same(yo, y, c["dtype"]), c


def test_fixture_poisons_only_its_own_group():
    z, cases = load_group()
    c = next(c for c in cases if c["kind"] == "sym" and c["dtype"] == "fp32" and c["group"] == 128)
    y = z[c["name"] + "_y"].reshape(2, -1, 128)
    assert np.isnan(y[0, 0]).all() and not np.isnan(y[0, 2]).any()


def test_grouped_dequantize_on_cpu_tensors():
    """QuantExport with [rows, C / g, 2] scales: dequantize() of the oracle's bins on the view equals the reference's group forward"""
    from llm_qat_amd import ops
    from oracle import oracle as O
    z, cases = load_group()
    dts = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
    for c in cases:
        if c["bits"] not in (4, 8) or c["dtype"] == "fp16" and c["kind"] == "sym" and c["bits"] == 8:
            continue
        x, y = z[c["name"] + "_x"], z[c["name"] + "_y"]
        g = c["group"]
        rows, cols = x.shape
        container = ops.default_container(c["kind"], c["bits"], dts[c["dtype"]])
        bins, scales, overflow = O.export(c["kind"], x.reshape(-1, g), rows * cols // g, g, c["bits"], container, c["dtype"])
        live = (overflow.reshape(rows, cols // g) == 0)
        if container == "int4":
            braw = torch.from_numpy(bins.reshape(rows, cols // 2).copy())
        else:
            braw = torch.from_numpy(bins.copy()).view(torch.int8 if container == "int8" else torch.int16).reshape(rows, cols)
            if c["kind"] == "asym" and container == "int8":
                braw = braw.view(torch.uint8)
        e = ops.QuantExport(kind=c["kind"], bins=braw, scales=torch.from_numpy(scales.copy()).view(rows, cols // g, 2),
                            overflow=torch.from_numpy(overflow.copy()).view(rows, cols // g), container=container, num_bits=c["bits"],
                            shape=(rows, cols), rows=rows, cols=cols, dtype=dts[c["dtype"]], group_size=g)
        d = e.dequantize()
        d = d.view(torch.int16).numpy().view(np.uint16) if c["dtype"] != "fp32" else d.numpy()
        d, yy = d.reshape(rows, cols // g, g), y.reshape(rows, cols // g, g)
        for r in range(rows):
            for k in range(cols // g):
                if not live[r, k] or np.isnan(yy[r, k].astype(np.float32) if c["dtype"] == "fp32" else 0).any():
                    continue
                a = d[r, k].view(np.uint32 if c["dtype"] == "fp32" else np.uint16)
                b = yy[r, k].view(np.uint32 if c["dtype"] == "fp32" else np.uint16)
                mask = 0x7FFFFFFF if c["dtype"] == "fp32" else 0x7FFF     # a zero bin dequantizes to +0 where the reference has -0
                same = (a == b) | (((a & mask) == 0) & ((b & mask) == 0))
                assert same.all(), (c, r, k)


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "models", "utils_quant.py")), reason="the reference is not on this machine")
def test_grouped_quantize_linear_on_cpu_tensors_equals_reference_on_views():
    sys.path.insert(0, REF)
    try:
        from models.utils_quant import SymQuantizer as RefSym
    finally:
        sys.path.remove(REF)
    import llm_qat_amd
    from llm_qat_amd import cpu_tensors
    prev = cpu_tensors.ENABLED
    llm_qat_amd.allow_cpu_tensors(True)
    try:
        torch.manual_seed(0)
        for act_g in (None, 64):
            m = llm_qat_amd.QuantizeLinear(256, 32, w_bits=4, a_bits=8, weight_group_size=128, act_group_size=act_g)
            with torch.no_grad():
                m.weight.copy_(torch.randn(32, 256) * 0.05)
            x = torch.randn(3, 5, 256, requires_grad=True)
            out = m(x)
            out.square().sum().backward()
            clip = torch.tensor([-2.0, 2.0])
            w = m.weight.detach().clone().requires_grad_(True)
            xr = x.detach().clone().requires_grad_(True)
            wq = RefSym.apply(w.reshape(-1, 128), clip, 4, False).reshape(w.shape)
            xq = RefSym.apply(xr, clip, 8, False) if act_g is None else RefSym.apply(xr.reshape(-1, act_g), clip, 8, False).reshape(xr.shape)
            ref = torch.nn.functional.linear(xq, wq)
            ref.square().sum().backward()
            assert torch.equal(out, ref)
            assert torch.equal(x.grad, xr.grad) and torch.equal(m.weight.grad, w.grad)
    finally:
        llm_qat_amd.allow_cpu_tensors(prev)
