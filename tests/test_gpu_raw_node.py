"""GPU tier: the one record (`_Raw`) and the one Python node (`_SharedAct`) behind every precomputed fake-quant result -- the weight cache's
value, K and V of a K + V launch, the cache route's activation.  The weight cache against no cache, bit for bit, in every backward mode,
with and without autocast and activation checkpointing and from either fill (the pair launch, `_quantized_weight`); an fp64 weight; the
in-place guard on the cache's node; the cache's node telling its forward thread that a backward started; quantize_kv against the unchanged
hooks.  Shapes are tests/test_gpu_pair_routes.py's: weight [128, 256], input [2, 3, 256], bf16, two weight elements beyond the STE clip."""
import os
import sys

import pytest
import torch
from torch.utils.checkpoint import checkpoint

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pair_routes import D_IN, D_OUT, mk, mk_input, same  # noqa: E402

# checkpoint -> (wcache_fill, wcache_hit) of one forward + backward with the cache on, from either fill, in every backward mode, with and
# without autocast: taken from the code as it stood before the cache stored a `_Raw` (the first pass fills, the recompute pass hits)
FILL_HIT = {None: (1, 0), "reentrant": (1, 1), "non_reentrant": (1, 1)}


@pytest.fixture()
def pkg():
    import llm_qat_amd
    assert llm_qat_amd.host_node() == "c++", llm_qat_amd.host_node()
    yield llm_qat_amd
    llm_qat_amd.cpp_node(True)
    llm_qat_amd.set_backward_mode("mask")
    llm_qat_amd.pair_operands(True)
    llm_qat_amd.inplace_weight_grad(True)
    llm_qat_amd.enable_weight_quant_cache(False)
    llm_qat_amd.reset_learned_state()


def step(pkg, cache, autocast, ckpt=None, dtype=torch.bfloat16, need_x=True):
    """one forward + backward of a fresh module -> ([output, input gradient, weight gradient], stats() delta)"""
    from llm_qat_amd import utils_quant as U
    pkg.reset_learned_state()
    pkg.enable_weight_quant_cache(cache)
    try:
        m, x = mk(U, dtype, 0), mk_input(False, False).to(dtype).requires_grad_(need_x)
        pkg.stats(reset=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = m(x) if ckpt is None else checkpoint(m, x, use_reentrant=ckpt == "reentrant")
        y.float().square().sum().backward()
        torch.cuda.synchronize()
        return [y.detach(), x.grad, m.weight.grad], pkg.stats(reset=True)
    finally:
        pkg.enable_weight_quant_cache(False)


@pytest.mark.parametrize("ckpt", [None, "reentrant", "non_reentrant"])
@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("mode", ["mask", "bounds", "plain"])
def test_weight_cache_equals_no_cache(pkg, mode, autocast, ckpt):
    pkg.set_backward_mode(mode)
    for pair in (True, False):      # the cache filled from the pair launch (mask mode) / from _quantized_weight
        pkg.pair_operands(pair)
        want, _ = step(pkg, False, autocast, ckpt)
        got, st = step(pkg, True, autocast, ckpt)
        print(mode, autocast, ckpt, pair, sorted(st.items()))
        assert all(same(a, b) for a, b in zip(got, want)), (mode, autocast, ckpt, pair)
        gw = got[2]
        assert gw[1, 3] == 0 and gw[D_OUT - 1, D_IN - 1] == 0 and gw.count_nonzero() > gw.numel() // 2, "the out-of-clip weight gradients are masked"
        assert (st.get("wcache_fill", 0), st.get("wcache_hit", 0)) == FILL_HIT[ckpt], (mode, autocast, ckpt, pair, st)
        assert st.get("pair_launch", 0) == (1 if pair and mode == "mask" else 0), st


def test_fp64_weight_with_the_cache(pkg):
    """float64 takes the saved-input data flow with the cache on as without it: the same bits"""
    for pair in (True, False):
        pkg.pair_operands(pair)
        want, _ = step(pkg, False, False, dtype=torch.float64)
        got, st = step(pkg, True, False, dtype=torch.float64)
        assert st.get("wcache_fill") == 1, st
        assert all(same(a, b) for a, b in zip(got, want)), pair
        assert got[2][1, 3] == 0 and got[2][D_OUT - 1, D_IN - 1] == 0


@pytest.mark.parametrize("pair", [True, False])
def test_cached_weight_gradient_is_masked_in_place(pkg, pair):
    """the cache's node masks F.linear's fresh wgrad where it stands, once, under the guard; the copying launch gives the same bits"""
    pkg.cpp_node(False)     # (the pair's C++ node counts its own in-place gradients: with the Python nodes the cached weight's is the only one)
    pkg.pair_operands(pair)
    got, st = step(pkg, True, False)
    assert st.get("inplace_taken") == 1 and not any(k.startswith("inplace_refused") for k in st), st
    pkg.inplace_weight_grad(False)
    want, st = step(pkg, True, False)
    assert not st.get("inplace_taken"), st
    assert all(same(a, b) for a, b in zip(got, want))


def test_cached_weight_backward_lets_go_of_remembered_activations(pkg):
    """the second use of a cached weight, input without a gradient: the cache's node is the only fake-quant node of the graph, and its
    backward tells its forward thread that a backward started, as every other fake-quant backward does"""
    from llm_qat_amd import utils_quant as U
    pkg.reset_learned_state()
    pkg.enable_weight_quant_cache(True)
    m, x = mk(U, torch.bfloat16, 0), mk_input(False, False)
    with torch.no_grad():
        m(x)
    pkg.stats(reset=True)
    y = m(x)
    assert pkg.stats().get("wcache_hit") == 1 and U._state().acts
    y.float().square().sum().backward()
    assert not U._state().acts
    assert m.weight.grad[1, 3] == 0 and m.weight.grad.count_nonzero() > 0


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("impl", ["c++", "python"])
def test_quantize_kv_equals_the_hooks(pkg, impl, autocast):
    """quantize_kv and the two unchanged hooks on the same [1, 8, 256] K and V: one helper behind both -- equal results, equal gradient
    dtypes (fp32 for the fp32 results under autocast, bf16 otherwise; bf16 for K and V themselves), equal one-tensor backward counts"""
    from llm_qat_amd import utils_quant as U
    assert pkg.cpp_node(impl == "c++") == (impl == "c++")
    clip = torch.tensor([-2.0, 2.0])
    res = {}
    for how in ("hooks", "explicit"):
        pkg.reset_learned_state()
        kp, vp = [U.QuantizeLinear(D_IN, D_IN, w_bits=4, a_bits=8).cuda().bfloat16() for _ in range(2)]
        with torch.no_grad():
            for s, p in enumerate((kp, vp)):
                p.weight.copy_((torch.randn(D_IN, D_IN, generator=torch.Generator().manual_seed(90 + s)) * 0.2).cuda().bfloat16())
        h = (torch.randn(1, 8, D_IN, generator=torch.Generator().manual_seed(7)) * 1.5).cuda().bfloat16().requires_grad_(True)
        dtypes = {}
        pkg.stats(reset=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            k, v = kp(h), vp(h)
            k.retain_grad(), v.retain_grad()
            if how == "hooks":
                kq = U.SymQuantizer.apply(k, clip, 8, False)
                vq = U.SymQuantizer.apply(v, clip, 8, False)
            else:
                kq, vq = U.quantize_kv(k, v, clip, clip, 8)
        kq.register_hook(lambda g: dtypes.__setitem__("kq", g.dtype))
        vq.register_hook(lambda g: dtypes.__setitem__("vq", g.dtype))
        (kq.float().square().sum() + 2 * vq.float().square().sum()).backward()
        torch.cuda.synchronize()
        st = pkg.stats(reset=True)
        dtypes["k"], dtypes["v"] = k.grad.dtype, v.grad.dtype
        res[how] = ([kq.detach(), vq.detach(), k.grad, v.grad, h.grad, kp.weight.grad, vp.weight.grad], dtypes,
                    (st.get("cpp_one_backward", 0), st.get("cpp_one_backward_wide", 0)), st)
    (a, da, ca, sta), (b, db, cb, _) = res["hooks"], res["explicit"]
    print(impl, autocast, da, ca, sorted(sta.items()))
    assert sta.get("kv_pair_launch") == 1 and sta.get("kv_pair_hit") == 1, sta
    assert all(same(p, q) for p, q in zip(a, b))
    wide = torch.float32 if autocast else torch.bfloat16
    assert da == db == {"kq": wide, "vq": wide, "k": torch.bfloat16, "v": torch.bfloat16}, (da, db)
    assert a[0].dtype == wide and a[1].dtype == wide
    assert ca == cb == (((0, 2) if autocast else (2, 0)) if impl == "c++" else (0, 0)), (ca, cb)
