"""CPU tier: the stateful host logic of the drop-in (activation sharing between sibling projections, the per-thread memory, the fail-closed
switches) exercised on CPU tensors (`allow_cpu_tensors`), against the same programs on the eager chain -- the sharing logic does not care
which device computed the values.  ADVICE r04 (medium): sibling modules over one input must be backward-able separately, without
retain_graph, as in the reference where every module has its own node.  GPU twins: tests/test_gpu_share_sequences.py, test_gpu_fail_closed.py.
"""
import gc
import os
import sys
import threading
import weakref

import pytest
import torch
from torch.utils.checkpoint import checkpoint

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_llama as TL  # noqa: E402


@pytest.fixture()
def UQ():
    import llm_qat_amd
    import llm_qat_amd.utils_quant as U
    llm_qat_amd.allow_cpu_tensors(True)
    llm_qat_amd.reset_learned_state()
    llm_qat_amd.stats(reset=True)
    yield U
    llm_qat_amd.allow_cpu_tensors(False)
    llm_qat_amd.conservative(False)
    llm_qat_amd.reset_learned_state()


def mk(Q, seed, ab=8, dtype=torch.float32):
    m = Q.QuantizeLinear(48, 48, w_bits=4, a_bits=ab).to(dtype)
    with torch.no_grad():
        m.weight.copy_((torch.randn(48, 48, generator=torch.Generator().manual_seed(60 + seed)) * 0.4).to(dtype))
    return m


def X(dtype=torch.float32):
    return (torch.randn(2, 7, 48, generator=torch.Generator().manual_seed(9)) * 1.5).to(dtype).requires_grad_(True)


def separate_backwards_no_retain(Q, dt):
    m0, m1, x = mk(Q, 0, dtype=dt), mk(Q, 1, dtype=dt), X(dt)
    a, b = m0(x), m1(x)
    a.sum().backward()
    g1 = x.grad.clone()
    b.sum().backward()
    return [a.detach(), b.detach(), g1, x.grad, m0.weight.grad, m1.weight.grad]


def later_consumer(Q, dt):
    ms, x = [mk(Q, 0, 8, dt), mk(Q, 1, 4, dt), mk(Q, 2, 8, dt)], X(dt)
    outs = [m(x) for m in ms]
    (sum(o.float().sum() * (i + 1) for i, o in enumerate(outs)) + (x * 3.0).float().sum()).backward()
    return [o.detach() for o in outs] + [m.weight.grad for m in ms] + [x.grad]


def checkpoint_around_one_sibling(Q, dt):
    q, k, v, x = mk(Q, 0, dtype=dt), mk(Q, 1, dtype=dt), mk(Q, 2, dtype=dt), X(dt)
    h = x * 1.0
    a = q(h)
    b = checkpoint(k, h, use_reentrant=False)
    c = v(h)
    (a.float() + 2 * b.float() + 3 * c.float()).sum().backward()
    return [a.detach(), b.detach(), c.detach(), x.grad, q.weight.grad, k.weight.grad, v.weight.grad]


def data_write_then_sibling(Q, dt):
    m0, m1, x = mk(Q, 0, dtype=dt), mk(Q, 1, dtype=dt), X(dt).detach()
    m0(x)
    x.mul_(0.5)            # an ordinary in-place write: bumps the version counter, the second sibling must see the new values
    return [m1(x)]


PROGRAMS = [separate_backwards_no_retain, later_consumer, checkpoint_around_one_sibling, data_write_then_sibling]


def fq_nodes(outs):
    """the distinct fake-quant autograd nodes that feed x into the GEMMs behind `outs` (walked with the node objects held: ids of
    temporaries get reused)"""
    seen, found, todo = [], [], [o.grad_fn for o in outs]
    while todo:
        n = todo.pop()
        if n is None or any(n is s for s in seen):
            continue
        seen.append(n)
        if any(k in type(n).__name__ for k in ("_SharedAct", "_PairNode")):   # the nodes an activation's gradient passes through
            found.append(n)
            continue
        todo.extend(f for f, _ in n.next_functions)
    return found


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: p.__name__)
def test_sharing_sequences_equal_the_eager_chain(UQ, prog, dt):
    import llm_qat_amd
    want = prog(TL.EagerQuant(), dt)
    for conservative in (False, True):
        llm_qat_amd.conservative(conservative)
        llm_qat_amd.reset_learned_state()
        assert same(want, prog(UQ, dt)), (prog.__name__, conservative)


def test_sharing_engages_on_the_default_path(UQ):
    import llm_qat_amd
    ms, x = [mk(UQ, i) for i in range(3)], X()
    outs = [m(x) for m in ms]
    st = llm_qat_amd.stats()
    assert st.get("act_share_miss") == 1 and st.get("act_share_hit") == 2, st
    assert len(fq_nodes(outs)) == 3, "sibling projections share an autograd node"


@pytest.mark.parametrize("prog", PROGRAMS, ids=lambda p: p.__name__)
def test_without_the_region_api_nothing_is_remembered(UQ, prog, monkeypatch):
    """torch._C._autograd._top_saved_tensors_default_hooks missing: fail CLOSED (rounds 1-4: `region is _region()` was then always true,
    i.e. the pre-fix behaviour that raised CheckpointError around one sibling)"""
    import llm_qat_amd
    want = prog(TL.EagerQuant(), torch.float32)
    monkeypatch.setattr(UQ, "_top_hooks", None)
    llm_qat_amd.reset_learned_state()
    llm_qat_amd.stats(reset=True)
    assert same(want, prog(UQ, torch.float32))
    st = llm_qat_amd.stats()
    assert st.get("share_disabled:no_region_api", 0) > 0 and not st.get("act_share_hit") and not st.get("act_share_miss"), st


def test_a_finished_thread_leaves_nothing_behind(UQ):
    refs = []

    def work():
        m0, m1, x = mk(UQ, 0), mk(UQ, 1), X().detach()
        with torch.no_grad():
            m0(x), m1(x)
        st = UQ._state()
        assert st.acts
        refs.append(weakref.ref(st))
        refs.extend(weakref.ref(e[3].out) for e in st.acts.values())

    t = threading.Thread(target=work)
    t.start()
    t.join()
    gc.collect()
    assert refs and all(r() is None for r in refs)


def test_a_backward_lets_go_of_what_its_forward_thread_remembered(UQ):
    m0, m1, x = mk(UQ, 0), mk(UQ, 1), X()
    a, b = m0(x), m1(x)
    st = UQ._state()
    assert st.acts
    held = [weakref.ref(e[3].out) for e in st.acts.values()]
    (a.sum() + b.sum()).backward()
    assert not st.acts and st.epoch >= 1
    del a, b
    gc.collect()
    assert all(r() is None for r in held), "the shared activation outlived its forward pass"


def _siblings_step(Q):
    """two sibling QuantizeLinear(64, 32) over one [3, 64] input that needs a gradient -> (outputs, gradients)"""
    ms = []
    for seed in (0, 1):
        m = Q.QuantizeLinear(64, 32, w_bits=4, a_bits=8)
        with torch.no_grad():
            m.weight.copy_(torch.randn(32, 64, generator=torch.Generator().manual_seed(80 + seed)) * 0.4)
        ms.append(m)
    x = (torch.randn(3, 64, generator=torch.Generator().manual_seed(11)) * 1.5).requires_grad_(True)
    return ms, x


def test_remembered_records_are_plain_data(UQ):
    """a `_Raw` is made with grad mode off: what `_ThreadState.acts` keeps carries no graph (it pinned the op chain's intermediates and the
    input until the entry was replaced), a sibling still finds it, and everything equals the conservative run bit for bit"""
    import llm_qat_amd
    llm_qat_amd.conservative(True)
    ms, x = _siblings_step(UQ)
    outs = [m(x) for m in ms]
    (outs[0].sum() + 2 * outs[1].sum()).backward()
    want = [o.detach() for o in outs] + [x.grad] + [m.weight.grad for m in ms]
    llm_qat_amd.conservative(False)
    llm_qat_amd.reset_learned_state()
    llm_qat_amd.stats(reset=True)
    ms, x = _siblings_step(UQ)
    a = ms[0](x)
    acts = UQ._state().acts
    assert acts, "nothing was remembered"
    for ent in acts.values():
        assert ent[3].out.grad_fn is None and ent[3].out.requires_grad is False, ent[3].out
    b = ms[1](x)
    st = llm_qat_amd.stats()
    assert st.get("act_share_miss") == 1 and st.get("act_share_hit") == 1, st
    for ent in UQ._state().acts.values():
        assert ent[3].out.grad_fn is None and ent[3].out.requires_grad is False, ent[3].out
    (a.sum() + 2 * b.sum()).backward()
    assert same(want, [a.detach(), b.detach(), x.grad] + [m.weight.grad for m in ms])


@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_a_quantizers_record_is_plain_data(UQ, kind):
    """the same for SymQuantizer.apply / AsymQuantizer.apply on a [3, 64] tensor: the record made outside a Function.forward has no graph,
    nothing with one is remembered, and result and gradient equal the conservative run bit for bit"""
    import llm_qat_amd
    quantizer = UQ.SymQuantizer if kind == "sym" else UQ.AsymQuantizer
    clip = torch.tensor([-2.0, 2.0])

    def run():
        x = (torch.randn(3, 64, generator=torch.Generator().manual_seed(12)) * 1.5).requires_grad_(True)
        y = quantizer.apply(x, clip, 8, False)
        (y * torch.arange(64.0)).sum().backward()
        return [y.detach(), x.grad]

    llm_qat_amd.conservative(True)
    want = run()
    llm_qat_amd.conservative(False)
    llm_qat_amd.reset_learned_state()
    x = (torch.randn(3, 64, generator=torch.Generator().manual_seed(12)) * 1.5).requires_grad_(True)
    raw = UQ._compute_raw(kind, x, clip, 8, False, False, True)
    assert raw.out.grad_fn is None and raw.out.requires_grad is False
    assert same(want, run())
    for ent in UQ._state().acts.values():
        assert ent[3].out.grad_fn is None and ent[3].out.requires_grad is False
