"""GPU tier: every route QuantizeLinear's operand pair can take -- the planned fast path, the general route (strided operands, the weight
cache), autocast, the dtype mix that is not paired, operands without a gradient, a sibling hit on either route -- under the C++ nodes and
the Python nodes.  Outputs and gradients are the eager chain's bits on every route; what each route launched, counted and saved is written
out below as literals (llm_qat_amd.stats() deltas over forward + backward; the tensors a saved_tensors_hooks recorder sees during the
forward, F.linear's own included), taken from the code as it stood before the routes were merged (since the weight cache keeps the
same record as every other route, its node saves the weight's one side buffer, as the planned route does, not the buffer's two views)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_llama as TL  # noqa: E402

D_IN, D_OUT = 256, 128      # 256 columns: 16-byte aligned rows; the launch shapes are test_gpu_row_launch_shapes.py's business

# name -> (strided input, weight cache ["first" / "second" use], autocast, weight dtype, need_w, need_x, sibling)
CASES = {
    "planned":              (False, None, False, torch.bfloat16, True, True, False),
    "strided":              (True, None, False, torch.bfloat16, True, True, False),
    "wcache_first":         (False, "first", False, torch.bfloat16, True, True, False),
    "wcache_second":        (False, "second", False, torch.bfloat16, True, True, False),
    "autocast":             (False, None, True, torch.bfloat16, True, True, False),
    "autocast_fp16_weight": (False, None, True, torch.float16, True, True, False),
    "input_without_grad":   (False, None, False, torch.bfloat16, True, False, False),
    "weight_frozen":        (False, None, False, torch.bfloat16, False, True, False),
    "both_frozen":          (False, None, False, torch.bfloat16, False, False, False),
    "sibling_planned":      (False, None, False, torch.bfloat16, True, True, True),
    "sibling_strided":      (True, None, False, torch.bfloat16, True, True, True),
}

# name -> node -> (stats() delta over forward + backward, [(shape, dtype) of every tensor saved during the forward, in order])
EXPECT = {'planned': {'c++': ({'act_share_miss': 1, 'cpp_pair_backward': 1, 'cpp_pair_forward': 1, 'inplace_taken': 1, 'pair_launch': 1},
                     [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
             'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1},
                        [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'strided': {'c++': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1},
                     [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
             'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1},
                        [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'wcache_first': {'c++': ({'act_share_miss': 1, 'cpp_one_backward': 1, 'inplace_taken': 1, 'pair_launch': 1, 'wcache_fill': 1},
                          [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
                  'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1, 'wcache_fill': 1},
                             [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'wcache_second': {'c++': ({'act_share_miss': 1, 'inplace_taken': 1, 'single_launch': 1, 'wcache_hit': 1},
                           [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
                   'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'single_launch': 1, 'wcache_hit': 1},
                              [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'autocast': {'c++': ({'act_share_miss': 1, 'cpp_pair_backward': 1, 'cpp_pair_forward': 1, 'inplace_taken': 1, 'pair_launch': 1},
                      [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
              'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1},
                         [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'autocast_fp16_weight': {'c++': ({'act_share_miss': 1, 'inplace_taken': 1, 'single_launch': 1},
                                  [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')]),
                          'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'single_launch': 1},
                                     [((5120,), 'uint8'), ((240,), 'uint8'), ((256, 128), 'bfloat16'), ((6, 256), 'bfloat16')])},
 'input_without_grad': {'c++': ({'act_share_miss': 1, 'cpp_pair_forward': 1, 'cpp_slow_backward': 1, 'pair_launch': 1},
                                [((5120,), 'uint8'), ((6, 256), 'bfloat16')]),
                        'python': ({'act_share_miss': 1, 'inplace_taken': 1, 'pair_launch': 1}, [((5120,), 'uint8'), ((6, 256), 'bfloat16')])},
 'weight_frozen': {'c++': ({'act_share_miss': 1, 'cpp_pair_forward': 1, 'cpp_slow_backward': 1, 'pair_launch': 1},
                           [((240,), 'uint8'), ((256, 128), 'bfloat16')]),
                   'python': ({'act_share_miss': 1, 'pair_launch': 1}, [((240,), 'uint8'), ((256, 128), 'bfloat16')])},
 'both_frozen': {'c++': ({'act_share_miss': 1, 'cpp_pair_forward': 1, 'pair_launch': 1}, []),
                 'python': ({'act_share_miss': 1, 'pair_launch': 1}, [])},
 'sibling_planned': {'c++': ({'act_share_hit': 1,
                              'act_share_miss': 1,
                              'cpp_pair_backward': 2,
                              'cpp_pair_forward': 1,
                              'cpp_weight_forward': 1,
                              'inplace_taken': 2,
                              'pair_launch': 1,
                              'single_launch': 1},
                             [((5120,), 'uint8'),
                              ((240,), 'uint8'),
                              ((256, 128), 'bfloat16'),
                              ((6, 256), 'bfloat16'),
                              ((5120,), 'uint8'),
                              ((240,), 'uint8'),
                              ((256, 128), 'bfloat16'),
                              ((6, 256), 'bfloat16')]),
                     'python': ({'act_share_hit': 1, 'act_share_miss': 1, 'inplace_taken': 2, 'pair_launch': 1, 'single_launch': 1},
                                [((5120,), 'uint8'),
                                 ((240,), 'uint8'),
                                 ((256, 128), 'bfloat16'),
                                 ((6, 256), 'bfloat16'),
                                 ((5120,), 'uint8'),
                                 ((240,), 'uint8'),
                                 ((256, 128), 'bfloat16'),
                                 ((6, 256), 'bfloat16')])},
 'sibling_strided': {'c++': ({'act_share_hit': 1, 'act_share_miss': 1, 'inplace_taken': 2, 'pair_launch': 1, 'single_launch': 1},
                             [((5120,), 'uint8'),
                              ((240,), 'uint8'),
                              ((256, 128), 'bfloat16'),
                              ((6, 256), 'bfloat16'),
                              ((5120,), 'uint8'),
                              ((240,), 'uint8'),
                              ((256, 128), 'bfloat16'),
                              ((6, 256), 'bfloat16')]),
                     'python': ({'act_share_hit': 1, 'act_share_miss': 1, 'inplace_taken': 2, 'pair_launch': 1, 'single_launch': 1},
                                [((5120,), 'uint8'),
                                 ((240,), 'uint8'),
                                 ((256, 128), 'bfloat16'),
                                 ((6, 256), 'bfloat16'),
                                 ((5120,), 'uint8'),
                                 ((240,), 'uint8'),
                                 ((256, 128), 'bfloat16'),
                                 ((6, 256), 'bfloat16')])}}


def mk(Q, dtype, seed):
    m = Q.QuantizeLinear(D_IN, D_OUT, w_bits=4, a_bits=8).cuda().to(dtype)
    with torch.no_grad():
        m.weight.copy_((torch.randn(D_OUT, D_IN, generator=torch.Generator().manual_seed(70 + seed)) * 0.5).cuda().to(dtype))
        m.weight[1, 3], m.weight[D_OUT - 1, D_IN - 1] = 2.5, -3.0     # beyond the STE clip: these gradients are masked
    return m


def mk_input(strided, need_x):
    base = (torch.randn(2, 6, D_IN, generator=torch.Generator().manual_seed(3)) * 1.4).cuda().bfloat16()
    x = base[:, ::2] if strided else base[:, ::2].contiguous()      # the same values on either route
    assert x.is_contiguous() != strided and x.shape == (2, 3, D_IN)
    return x.requires_grad_(need_x)


def forward_backward(mods, x, autocast, saved=None):
    def pack(t):
        saved.append((tuple(t.shape), str(t.dtype).replace("torch.", "")))
        return t
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        if saved is None:
            ys = [m(x) for m in mods]
        else:
            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                ys = [m(x) for m in mods]
    if any(y.requires_grad for y in ys):
        sum(y.float().square().sum() for y in ys).backward()
    return [y.detach() for y in ys] + [x.grad] + [m.weight.grad for m in mods]


def run_case(pkg, Q, name):
    """-> (outputs and gradients, stats delta, saved tensors) of one case with Q's QuantizeLinear (utils_quant or the eager twin)"""
    strided, wcache, autocast, wdtype, need_w, need_x, sibling = CASES[name]
    pkg.reset_learned_state()
    pkg.enable_weight_quant_cache(wcache is not None)
    try:
        mods = [mk(Q, wdtype, s) for s in range(2 if sibling else 1)]
        for m in mods:
            m.weight.requires_grad_(need_w)
        if wcache == "second":      # the first use of the step fills the cache; the use under test finds it
            forward_backward(mods, mk_input(strided, need_x), autocast)
            for m in mods:
                m.weight.grad = None
        saved = []
        pkg.stats(reset=True)
        res = forward_backward(mods, mk_input(strided, need_x), autocast, saved)
        torch.cuda.synchronize()
        return res, pkg.stats(reset=True), saved
    finally:
        pkg.enable_weight_quant_cache(False)
        pkg.reset_learned_state()


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(a, b))


@pytest.fixture()
def pkg():
    import llm_qat_amd
    assert llm_qat_amd.host_node() == "c++", llm_qat_amd.host_node()
    llm_qat_amd.set_semantics("device_eager")
    yield llm_qat_amd
    llm_qat_amd.cpp_node(True)
    llm_qat_amd.set_semantics("cpu_eager")
    llm_qat_amd.reset_learned_state()


@pytest.fixture(scope="module")
def eager():
    """the eager chain's outputs and gradients per case, computed once on the device (read-only)"""
    import llm_qat_amd
    llm_qat_amd.set_semantics("device_eager")
    E = TL.EagerQuant()
    return {name: run_case(llm_qat_amd, E, name)[0] for name in CASES}


@pytest.mark.parametrize("impl", ["c++", "python"])
@pytest.mark.parametrize("name", list(CASES))
def test_route(pkg, eager, name, impl):
    from llm_qat_amd import utils_quant as U
    assert pkg.cpp_node(impl == "c++") == (impl == "c++")
    res, st, saved = run_case(pkg, U, name)
    print(name, impl, sorted(st.items()), saved)
    want = eager[name]
    assert len(res) == len(want) and all(same(a, b) for a, b in zip(res, want)), (name, impl)
    want_st, want_saved = EXPECT[name][impl]
    assert st == want_st, (name, impl, st)
    assert saved == want_saved, (name, impl, saved)


@pytest.mark.parametrize("impl", ["c++", "python"])
def test_routes_agree_with_each_other(pkg, impl):
    """the same values through the planned and the general route: the module's own outputs and gradients are one set of bits"""
    from llm_qat_amd import utils_quant as U
    assert pkg.cpp_node(impl == "c++") == (impl == "c++")
    got = {name: run_case(pkg, U, name)[0] for name in ("planned", "strided", "wcache_first", "wcache_second", "sibling_planned", "sibling_strided")}
    for a, b in (("planned", "strided"), ("planned", "wcache_first"), ("planned", "wcache_second"), ("sibling_planned", "sibling_strided")):
        assert len(got[a]) == len(got[b]) and all(same(p, q) for p, q in zip(got[a], got[b])), (impl, a, b)


def test_gradient_handed_back_from_cpp(pkg):
    """an fp32 gradient for the bf16 pair's output and a backward that is itself recorded (create_graph=True): the C++ node hands back to the
    Python node's code, counted, and gives its bits and the eager chain's"""
    from llm_qat_amd import utils_quant as U
    g32 = torch.randn(2, 3, D_OUT, generator=torch.Generator().manual_seed(5)).cuda()
    res = {}
    for impl in ("eager", "c++", "python"):
        Q = TL.EagerQuant() if impl == "eager" else U
        if impl != "eager":
            pkg.cpp_node(impl == "c++")
        pkg.reset_learned_state()
        m, x = mk(Q, torch.bfloat16, 0), mk_input(False, True)
        pkg.stats(reset=True)
        y = m(x)
        gx, gw = torch.autograd.grad(y, [x, m.weight], grad_outputs=g32, create_graph=True)
        ggx, = torch.autograd.grad(gx.float().square().sum() + gw.float().square().sum(), [x], allow_unused=True)
        res[impl] = (y.detach(), gx.detach(), gw.detach(), ggx)
        st = pkg.stats(reset=True)
        print(impl, sorted(st.items()))
        assert st.get("cpp_slow_backward", 0) == (1 if impl == "c++" else 0), (impl, st)
    for impl in ("c++", "python"):
        assert all(same(a, b) for a, b in zip(res[impl], res["eager"])), impl
