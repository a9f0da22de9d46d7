"""GPU tier of group-wise fake quantization (fq_group_fwd and everything above it), zero tolerance (any NaN equals any NaN):
the reference's group results (tests/golden/group.npz), the oracle and the row-wise kernels on the [rows * C / g, g] view, the live ATen
chain, training-mode side outputs in the full-row layout with the unchanged STE backwards, QuantizeLinear with group sizes (autocast,
checkpointing, torch.compile), the view route, the export and canary regions around every output."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
CLIP = torch.tensor([-2.0, 2.0])


@pytest.fixture(autouse=True)
def _semantics():
    import llm_qat_amd
    prev = llm_qat_amd.get_semantics()
    yield
    llm_qat_amd.set_semantics(prev)


def bits_of(t):
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def same(a, b):
    """zero tolerance, any NaN equals any NaN"""
    assert a.shape == b.shape and a.dtype == b.dtype
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return bool((bits_of(a) == bits_of(b))[~na.cpu().numpy()].all())


def counts():
    from llm_qat_amd import ops
    return dict(ops.group_counts)


def sample(shape, dt, seed, clip_rows=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(shape, generator=g, device=DEV) * 0.05
    flat = x.view(-1, shape[-1])
    flat[1, 5] = float("nan")
    flat[2, 7] = float("inf")
    flat[3, :300] = 0.0
    flat[3, 1] = -0.0
    if clip_rows:
        flat[5::7] *= 80.0          # rows that reach the clip
    return x.to(DTS[dt])


def test_group_fixture_through_the_kernel():
    import llm_qat_amd
    from llm_qat_amd import ops
    llm_qat_amd.set_semantics("cpu_eager")
    z = np.load(os.path.join(GOLDEN, "group.npz"))
    cases = json.loads(str(z["manifest"]))["cases"]
    before = counts()
    for c in cases:
        xn = z[c["name"] + "_x"]
        dt = DTS[c["dtype"]]
        x = torch.from_numpy(xn.astype(np.int16) if xn.dtype == np.uint16 else xn).view(dt).to(DEV)
        y = torch.from_numpy(z[c["name"] + "_y"].astype(np.int16) if xn.dtype == np.uint16 else z[c["name"] + "_y"]).view(dt)
        fn = ops.sym_quantize if c["kind"] == "sym" else ops.asym_quantize
        assert same(fn(x, c["bits"], group_size=c["group"]).cpu(), y), c
    assert counts()["group_launch"] - before["group_launch"] == len(cases)   # every fixture case is served by the kernel


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_kernel_equals_row_path_and_oracle_on_the_view(dt, kind):
    import llm_qat_amd
    from llm_qat_amd import ops
    from oracle import oracle as O
    fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
    shapes = [(4096, 11008), (11008, 4096), (2, 2048, 4096), (8, 256)] if dt == "bf16" else [(4096, 11008), (2, 256, 4096), (8, 256)]
    for si, shape in enumerate(shapes):
        x = sample(shape, dt, 10 + si)
        for sem in ("cpu_eager", "device_eager"):
            llm_qat_amd.set_semantics(sem)
            for g in ((32, 64, 128, 256) if dt != "fp32" else (64, 128, 256)):
                if shape[-1] % g:
                    continue
                for bits in (3, 4, 8, 16):
                    before = counts()["group_launch"]
                    y = fn(x, bits, group_size=g)
                    assert counts()["group_launch"] == before + 1
                    yr = fn(x.reshape(-1, g), bits).reshape(x.shape)
                    assert same(y, yr), (shape, sem, g, bits)
                    if sem == "cpu_eager" and bits == 4 and (x.numel() <= 2 ** 23 or g == 128):
                        xn = bits_of(x).view(np.uint16 if dt != "fp32" else np.float32).reshape(-1, g)
                        of = O.sym_fwd if kind == "sym" else O.asym_fwd
                        yo = of(xn, xn.shape[0], g, bits, dt, want_idx=False)[0]
                        yo_t = torch.from_numpy(yo.astype(np.int16) if dt != "fp32" else yo).view(DTS[dt]).reshape(x.shape)
                        assert same(y.cpu(), yo_t), (shape, g, bits)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_device_eager_and_autocast_equal_the_live_chain(dt):
    import llm_qat_amd
    from llm_qat_amd import ops
    from oracle import eager_chain as E
    llm_qat_amd.set_semantics("device_eager")
    x = sample((512, 4096), dt, 3)
    for g in (32, 128, 256):
        xv = x.reshape(-1, g)
        for bits in (4, 8):
            assert same(ops.sym_quantize(x, bits, group_size=g), E.sym_forward(xv, bits).reshape(x.shape))
            assert same(ops.asym_quantize(x, bits, group_size=g), E.asym_forward(xv, bits).reshape(x.shape))
            with torch.autocast("cuda", dtype=DTS[dt]):
                ref = E.sym_forward(xv, bits).to(DTS[dt]).reshape(x.shape)       # fp32 result, rounded once (F.linear's cast)
                before = counts()["group_launch"]
                res = ops.group_forward("sym", x, bits, g, autocast=True)
                assert counts()["group_launch"] == before + 1
            assert same(res[0], ref)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_training_mode_side_outputs_serve_the_unchanged_backward(dt, kind):
    from llm_qat_amd import ops
    from oracle import eager_chain as E
    x = sample((256, 4096), dt, 5, clip_rows=True)
    rows, cols = 256, 4096
    for g in (64, 128):
        res = ops.quantize_train(kind, x, 4, False, -2.0, 2.0, group_size=g)
        assert res is not None
        y, bounds, mask = res
        fn = ops.sym_quantize if kind == "sym" else ops.asym_quantize
        assert same(y, fn(x, 4, group_size=g))
        # full-row bounds and bitmap: what the row-wise training forward of the same tensor records
        _, rb, rm = ops.quantize_train(kind, x, 4, False, -2.0, 2.0)
        assert same(bounds, rb)
        xf = x.float()
        want_ub = xf.abs().amax(1) if kind == "sym" else xf.amax(1)
        assert same(bounds[:, 0], want_ub)
        clippable = ~((bounds[:, 0] < 2.0) & (bounds[:, 1] > -2.0))
        assert clippable.any() and (~clippable).any()
        mw = cols // 64 * 8
        m1, m2 = mask.view(rows, mw)[clippable], rm.view(rows, mw)[clippable]
        assert torch.equal(m1, m2)
        pred = ((x >= 2.0) | (x <= -2.0))[clippable]
        bitsv = torch.from_numpy(np.unpackbits(m1.cpu().numpy(), axis=1, bitorder="little").astype(bool))
        assert torch.equal(bitsv, pred.cpu())
        gout = torch.randn(x.shape, device=DEV).to(x.dtype)
        ref = E.ste_backward(gout, x, CLIP.to(DEV))
        assert same(ops.ste_backward_mask(gout, -2.0, 2.0, bounds, mask, rows, cols), ref)
        gin = gout.clone()
        out = ops.ste_backward_mask(gin, -2.0, 2.0, bounds, mask, rows, cols, inplace=True)
        assert out.data_ptr() == gin.data_ptr() and same(out, ref)
    # a weight whose rows never reach the clip is not touched in place
    w = (torch.randn(128, 4096, device=DEV) * 0.02).to(DTS[dt])
    _, b, m = ops.quantize_train(kind, w, 4, False, -2.0, 2.0, group_size=128)
    gw = torch.randn(w.shape, device=DEV).to(w.dtype)
    keep = gw.clone()
    ops.ste_backward_mask(gw, -2.0, 2.0, b, m, 128, 4096, inplace=True)
    assert torch.equal(gw, keep)


class _EagerGroupLinear(torch.nn.Module):
    def __init__(self, w, wg, ag):
        super().__init__()
        self.weight = torch.nn.Parameter(w.detach().clone())
        self.wg, self.ag = wg, ag

    def forward(self, x):
        from oracle.eager_chain import EagerSym
        c = CLIP.to(x.device)
        wq = EagerSym.apply(self.weight.reshape(-1, self.wg), c, 4, False).reshape(self.weight.shape)
        xq = EagerSym.apply(x, c, 8, False) if self.ag is None else EagerSym.apply(x.reshape(-1, self.ag), c, 8, False).reshape(x.shape)
        return torch.nn.functional.linear(xq, wq)


@pytest.mark.parametrize("ag", [None, 128])
@pytest.mark.parametrize("mode", ["plain", "autocast", "checkpoint"])
def test_quantize_linear_grouped_equals_eager_chain_on_views(ag, mode):
    import llm_qat_amd
    from llm_qat_amd.utils_quant import QuantizeLinear
    from torch.utils.checkpoint import checkpoint
    llm_qat_amd.set_semantics("device_eager")
    torch.manual_seed(1)
    m = QuantizeLinear(4096, 1024, w_bits=4, a_bits=8, weight_group_size=128, act_group_size=ag).to(DEV).bfloat16()
    with torch.no_grad():
        m.weight.mul_(40.0)   # some weight rows reach the clip
    e = _EagerGroupLinear(m.weight, 128, ag)
    x0 = (torch.randn(2, 64, 4096, device=DEV) * 3).bfloat16()
    outs = []
    llm_qat_amd.stats(reset=True)
    for mod in (m, e):
        x = x0.clone().requires_grad_(True)
        if mode == "autocast":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = mod(x)
        elif mode == "checkpoint":
            out = checkpoint(mod, x, use_reentrant=False)
        else:
            out = mod(x)
        out.float().square().sum().backward()
        outs.append((out.detach(), x.grad, mod.weight.grad))
        if mod is m:
            st = llm_qat_amd.stats(reset=True)
    for a, b in zip(outs[0], outs[1]):
        assert same(a, b), mode
    n_fwd = 2 if mode == "checkpoint" else 1
    assert st.get("group_launch", 0) == n_fwd * (1 if ag is None else 2), st
    assert st.get("single_launch", 0) == n_fwd and not st.get("pair_launch") and not st.get("group_view_route"), st


def test_quantize_linear_grouped_compiled_equals_eager():
    from llm_qat_amd.utils_quant import QuantizeLinear
    torch.manual_seed(2)
    m = QuantizeLinear(512, 256, w_bits=4, a_bits=8, weight_group_size=128, act_group_size=64).to(DEV).bfloat16()
    x = (torch.randn(4, 512, device=DEV)).bfloat16()
    ref = m(x)
    cm = torch.compile(m, fullgraph=True)
    assert same(cm(x), ref)


def test_view_route_is_bit_identical_and_counted():
    from llm_qat_amd import ops
    x = sample((64, 4608), "bf16", 7)
    cases = [(x, 96), (x[:, :4096], 128), (x.double()[:, :4096].contiguous(), 128), (x[:, 1:4097].contiguous(), 16)]
    for t, g in cases:
        for kind, fn in (("sym", ops.sym_quantize), ("asym", ops.asym_quantize)):
            before = counts()
            y = fn(t, 4, group_size=g)
            after = counts()
            assert after["group_view_route"] == before["group_view_route"] + 1 and after["group_launch"] == before["group_launch"]
            assert same(y, fn(t.reshape(-1, g), 4).reshape(t.shape))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_export_weight_grouped(dt):
    import llm_qat_amd
    from llm_qat_amd import ops
    from llm_qat_amd.utils_quant import QuantizeLinear
    from oracle import oracle as O
    llm_qat_amd.set_semantics("cpu_eager")
    m = QuantizeLinear(4096, 256, w_bits=4, a_bits=8, weight_group_size=128).to(DEV).to(DTS[dt])
    e = m.export_weight()
    assert e.group_size == 128 and e.scales.shape == (256, 32, 2) and e.bins.shape == (256, 2048)
    w = m.weight.detach()
    wn = bits_of(w).view(np.uint16).reshape(-1, 128)
    bins, scales, overflow = O.export("sym", wn, wn.shape[0], 128, 4, "int4", dt)
    assert np.array_equal(e.bins.cpu().numpy().reshape(-1), bins.reshape(-1))
    assert np.array_equal(e.scales.cpu().numpy().reshape(-1, 2).view(np.uint32), scales.view(np.uint32))
    assert (e.overflow == 0).all()
    y = ops.sym_quantize(w, 4, group_size=128)
    d = e.dequantize()
    nz = y != 0        # (a zero bin dequantizes to +0 where the forward may have -0)
    assert torch.equal(d[nz], y[nz]) and (d[~nz] == 0).all()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_canaries_around_outputs(dt):
    from llm_qat_amd import _lib, ops
    L = _lib.lib()
    rows, cols, g = 64, 4096, 128
    es = 2 if dt == "bf16" else 4
    n = rows * cols
    pad = 4096
    x = sample((rows, cols), dt, 9, clip_rows=True)
    ybuf = torch.full((n + 2 * pad,), 7.0, device=DEV, dtype=DTS[dt])
    mb = L.fq_ste_mask_bytes(rows, cols, ops._DTYPES[x.dtype])
    mbuf = torch.full((mb + 2 * pad,), 0xA5, device=DEV, dtype=torch.uint8)
    bbuf = torch.full((rows * 2 + 2 * pad,), 3.0, device=DEV, dtype=torch.float32)
    y = ybuf[pad:pad + n]
    rc = L.fq_group_fwd(0, x.data_ptr(), y.data_ptr(), rows, cols, g, 4, ops._DTYPES[x.dtype], 0, 0, -2.0, 2.0, bbuf[pad:].data_ptr(),
                        mbuf[pad:].data_ptr(), mb, ops._stream(x))
    assert rc == 0, L.fq_last_error()
    torch.cuda.synchronize()
    assert (ybuf[:pad] == 7.0).all() and (ybuf[pad + n:] == 7.0).all()
    assert (mbuf[:pad] == 0xA5).all() and (mbuf[pad + mb:] == 0xA5).all()
    assert (bbuf[:pad] == 3.0).all() and (bbuf[pad + 2 * rows:] == 3.0).all()
    assert same(y.view(rows, cols), ops.sym_quantize(x.reshape(-1, g), 4).reshape(rows, cols))
