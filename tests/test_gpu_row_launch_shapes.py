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

import group_cases as C
import mx_rules_reference as R
from group_ntl_worker import DTS, from_dev, report, to_dev
from mx_reference import encode, pack_fp4
from mx_rot_reference import rotate_bits
from mx_rules_cases import rand_bits

pytestmark = pytest.mark.gpu

ROWS = 5
LO, HI = -2.0, 2.0
BITS = 4
# threads per row -> the nvec at the top of each of its rungs (fq_shapes.h by_reg_shape)
RUNGS = {64: (64, 128, 192), 128: (256, 384), 256: (512, 768), 512: (1024, 1536, 2048, 2560, 3072, 3584, 4096), 1024: (5120, 6144, 7168, 8192)}
NVECS = [n for tpr in RUNGS for n in RUNGS[tpr]]
# fp32-result forward (launch_wide): nh = cols / 4 half-vectors per row, hpt = ceil(nh / TPR) of them per thread; TPR 64 up to nh = 512,
# 256 up to 2048, then 1024.  nh = TPR * hpt - 2: the last slot is a clamped duplicate, and cols stays a multiple of 8 (the bitmap's unit).
WIDE_NH = [64 * h - 2 for h in range(1, 9)] + [256 * h - 2 for h in range(3, 9)] + [1024 * h - 2 for h in range(3, 9)]
# fp32-gradient backward (launch_ste_mask_wide): one chunk up to nh = 2048, hpt = ceil(nh / 256) = 1 .. 8 (the TPR 256 widths above are
# hpt 3 .. 8 of it; these are 1 and 2)
WIDE_BWD_NH = [256 * h - 2 for h in range(1, 9)]


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    llm_qat_amd.set_semantics("cpu_eager")
    yield
    llm_qat_amd.set_semantics(prev)


# ---- inputs and expected values: numpy and the oracle only, computed once per process -------------------------------------------------------

_memo = {}


def memo(fn):
    def wrapped(*key):
        k = (fn.__name__,) + key
        if k not in _memo:
            v = fn(*key)
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
            _memo[k] = v
        return _memo[k]
    return wrapped


@memo
def row_bits(dt, cols, rows=ROWS):
    """bit patterns [rows, cols]: even rows cross the clip +-2, odd rows stay well inside it; row 0 holds +-2 and the patterns one ulp on
    either side of them and a -0.0, some of them in the row's last vector; row 2 (if there is one) a NaN there"""
    u = C.uint_of(dt)
    rng = np.random.default_rng(cols * 7 + rows)
    v = rng.standard_normal((rows, cols)) * np.where(np.arange(rows) % 2 == 0, 1.5, 0.25)[:, None]
    b = encode(v.astype(np.float32).astype(np.float64), dt).astype(u)
    two, sign = u(C.TWO[dt]), u(C.SIGN[dt])
    edge = [two, two | sign, two + u(1), two - u(1), (two + u(1)) | sign, (two - u(1)) | sign, sign]
    where = [3, cols // 2, cols // 3, cols - 1, cols - 2, 0, cols - 3]
    for p, val in zip(where, edge):
        b[0, p] = val
    if rows > 2:
        b[2, cols - 4] = C.NAN[dt]
    return b


@memo
def forward_reference(dt, kind, cols, rows=ROWS):
    from oracle import oracle as O
    fn = O.sym_fwd if kind == "sym" else O.asym_fwd
    return fn(C.oracle_view(row_bits(dt, cols, rows), dt), rows, cols, BITS, dt, sem=0, want_idx=False)[0].view(C.uint_of(dt)).reshape(rows, cols)


@memo
def autocast_reference(dt, wide, cols, rows=ROWS):
    """the oracle the autocast tests use: bit patterns of the tensor dtype, or (wide) of the fp32 result"""
    from oracle import oracle as O
    y = O.sym_fwd_autocast(row_bits(dt, cols, rows), rows, cols, BITS, dt, wide=wide)[0]
    return y.view(np.uint32 if wide else np.uint16).reshape(rows, cols)


@memo
def side_reference(dt, asym, cols, rows=ROWS):
    """-> (bounds float32 [rows, 2] as bits, clippable rows, predicate bool [rows, cols])"""
    b = row_bits(dt, cols, rows)
    bounds = C.row_bounds(b, dt, asym)
    clippable = ~((bounds[:, 0] < HI) & (bounds[:, 1] > LO))
    assert clippable.any() and (~clippable).any()
    return bounds.view(np.uint32), clippable, C.clip_predicate(b, dt, LO, HI)


@memo
def grad_and_masked(dt, cols, rows=ROWS):
    """a gradient with NaN, +-Inf and -0.0 at zeroed and at kept positions, and that gradient with +0.0 where the predicate holds"""
    pred = C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI)
    g = C.grad_bits(pred, dt, cols + rows)
    want = g.copy()
    want[pred] = 0
    return g, want


@memo
def wide_grad_and_masked(dt, cols, rows=ROWS):
    """the fp32 gradient of a fp32-result forward, and its rounding to the input's dtype with +0.0 where the predicate holds"""
    g = C.grad_bits(C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI), "fp32", cols + rows)
    want = from_dev(torch.from_numpy(g.view(np.float32).copy()).to(DTS[dt]), dt).copy()
    want[C.clip_predicate(row_bits(dt, cols, rows), dt, LO, HI)] = 0
    return g, want


def unpack_mask(mask, rows, cols):
    m = mask.cpu().numpy().reshape(rows, -1)
    assert m.shape[1] == (cols + 63) // 64 * 8
    return np.unpackbits(m, axis=1, bitorder="little")[:, :cols].astype(bool)


def split(side, rows):
    return side[: rows * 8].view(torch.float32).view(rows, 2), side[rows * 8:]


def check_side(bounds, mask, dt, asym, cols, what, rows=ROWS):
    want_b, clippable, pred = side_reference(dt, asym, cols, rows)
    out = [report(from_dev(bounds, "fp32"), want_b, "fp32", f"{what} bounds")]
    got = unpack_mask(mask, rows, cols)
    if not np.array_equal(got[clippable], pred[clippable]):
        out.append(f"{what} bitmap differs from the predicate at {np.argwhere(got[clippable] != pred[clippable])[:4].tolist()}")
    return out


def none_failed(failures):
    failures = [f for f in failures if f]
    assert not failures, (len(failures), failures[:5])


# ---- forward: every rung of the register ladder ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_forward_plain_and_training_at_every_rung(dt, kind):
    from llm_qat_amd import ops
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        x = to_dev(row_bits(dt, cols), dt)
        want = forward_reference(dt, kind, cols)
        failures.append(report(from_dev(fn(x, BITS), dt), want, dt, f"{dt} {kind} nvec {nvec} plain"))
        res = ops.quantize_train(kind, x, BITS, False, LO, HI)
        assert res is not None, (dt, kind, nvec)
        y, bounds, mask = res
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} {kind} nvec {nvec} training"))
        failures += check_side(bounds, mask, dt, kind == "asym", cols, f"{dt} {kind} nvec {nvec}")
    none_failed(failures)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_narrow_at_every_rung(dt):
    from llm_qat_amd import ops
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        x = to_dev(row_bits(dt, cols), dt)
        want = autocast_reference(dt, False, cols)
        y = ops.sym_forward_autocast(x, BITS, False, wide=False)[0]
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} autocast nvec {nvec} plain"))
        y, side, rows, _, got = ops.sym_forward_autocast(x, BITS, False, wide=False, lo=LO, hi=HI, train="mask")
        assert got == "mask" and rows == ROWS, (dt, nvec, got)
        failures.append(report(from_dev(y, dt), want, dt, f"{dt} autocast nvec {nvec} training"))
        failures += check_side(*split(side, ROWS), dt, False, cols, f"{dt} autocast nvec {nvec}")
    none_failed(failures)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_autocast_wide_at_every_half_vector_count(dt):
    from llm_qat_amd import ops
    failures = []
    for nh in WIDE_NH + WIDE_BWD_NH[:2]:
        cols = nh * 4
        x = to_dev(row_bits(dt, cols), dt)
        want = autocast_reference(dt, True, cols)
        y = ops.sym_forward_autocast(x, BITS, False, wide=True)[0]
        assert y.dtype is torch.float32
        failures.append(report(from_dev(y, "fp32"), want, "fp32", f"{dt} wide nh {nh} plain"))
        y, side, _, _, got = ops.sym_forward_autocast(x, BITS, False, wide=True, lo=LO, hi=HI, train="mask")
        assert got == "mask", (dt, nh, got)
        failures.append(report(from_dev(y, "fp32"), want, "fp32", f"{dt} wide nh {nh} training"))
        failures += check_side(*split(side, ROWS), dt, False, cols, f"{dt} wide nh {nh}")
        # the fp32-gradient backward on that forward's side outputs: one slot, and two slots with a 3-row tensor of the same width
        g, want_g = wide_grad_and_masked(dt, cols)
        gout = to_dev(g, "fp32")
        failures.append(report(from_dev(ops.train_backward_wide(gout, side, ROWS, cols, LO, HI, DTS[dt]), dt), want_g, dt, f"{dt} wide nh {nh} backward"))
        if nh in WIDE_BWD_NH:
            x3 = to_dev(row_bits(dt, cols, 3), dt)
            side3 = ops.sym_forward_autocast(x3, BITS, False, wide=True, lo=LO, hi=HI, train="mask")[1]
            g3, want_g3 = wide_grad_and_masked(dt, cols, 3)
            o5, o3 = ops.pair_backward_wide(gout, to_dev(g3, "fp32"), side, side3, ROWS, 3, cols, LO, HI, DTS[dt])
            failures.append(report(from_dev(o5, dt), want_g, dt, f"{dt} wide nh {nh} backward, slot 0 of 2"))
            failures.append(report(from_dev(o3, dt), want_g3, dt, f"{dt} wide nh {nh} backward, slot 1 of 2"))
    none_failed(failures)


# ---- backward from (bounds, bitmap): every vector count in every launch form ---------------------------------------------------------------

def backward_vpt(nvec_row):
    """launch_ste_mask's vectors per thread for a row of nvec_row vectors"""
    chunks = (nvec_row + 2047) // 2048
    cv = ((nvec_row + chunks - 1) // chunks + 63) // 64 * 64
    return (cv + 255) // 256


def test_the_rung_widths_reach_every_backward_vector_count():
    assert {backward_vpt(n - 1) for n in NVECS} == set(range(1, 9))


@pytest.mark.parametrize("kind", ["sym", "asym"])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_mask_backward_one_tensor_and_in_place(dt, kind):
    from llm_qat_amd import ops
    failures = []
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        _, bounds, mask = ops.quantize_train(kind, to_dev(row_bits(dt, cols), dt), BITS, False, LO, HI)
        g, want = grad_and_masked(dt, cols)
        gout = to_dev(g, dt)
        failures.append(report(from_dev(ops.ste_backward_mask(gout, LO, HI, bounds, mask, ROWS, cols), dt), want, dt, f"{dt} {kind} nvec {nvec} backward"))
        gin = gout.clone()
        out = ops.ste_backward_mask(gin, LO, HI, bounds, mask, ROWS, cols, inplace=True)
        assert out.data_ptr() == gin.data_ptr()
        failures.append(report(from_dev(out, dt), want, dt, f"{dt} {kind} nvec {nvec} backward in place"))
    none_failed(failures)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_mask_backward_two_and_four_slot_forms(dt):
    """the two-slot form (pair_backward: both copying, and the first slot in place as a weight's gradient is) and the four-slot form
    (multi_backward with three tensors, the first in place): tensors of 5, 3 and 4 rows of the same width"""
    from llm_qat_amd import ops
    failures = []
    nrows = (ROWS, 3, 4)
    for nvec in NVECS:
        cols = (nvec - 1) * C.EPV[dt]
        sides = [ops.train_forward("sym", to_dev(row_bits(dt, cols, r), dt), BITS, False, LO, HI)[1] for r in nrows]
        gw = [grad_and_masked(dt, cols, r) for r in nrows]
        for inplace in (False, True):
            what = f"{dt} nvec {nvec} inplace {inplace}"
            g0, g1, g2 = (to_dev(g, dt) for g, _ in gw)
            o0, o1 = ops.pair_backward(g0, g1, sides[0], sides[1], nrows[0], nrows[1], cols, LO, HI, inplace_w=inplace)
            assert (o0.data_ptr() == g0.data_ptr()) == inplace
            failures.append(report(from_dev(o0, dt), gw[0][1], dt, f"{what} pair slot 0"))
            failures.append(report(from_dev(o1, dt), gw[1][1], dt, f"{what} pair slot 1"))
            g0 = to_dev(gw[0][0], dt)
            outs = ops.multi_backward([g0, g1, g2], sides, list(nrows), cols, LO, HI, inplace=[inplace, False, False])
            assert (outs[0].data_ptr() == g0.data_ptr()) == inplace
            for i, o in enumerate(outs):
                failures.append(report(from_dev(o, dt), gw[i][1], dt, f"{what} multi slot {i}"))
    none_failed(failures)


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
