"""CPU tier: which quantizer serves each operand of a QuantizeLinear (`_weight_route` / `_act_route`), over the full cross of the
constructor's settings, against a table written out by hand from the three ladders the module used to carry (the tail of `forward`,
`_forward_mx`, `_forward_compiled`: for every layer the constructor accepts they took the same decision) -- and that the three appliers
dispatch on exactly those tags.  No launch: the layers live on the CPU and the appliers' launch callables are recorders."""
import itertools

import pytest
import torch

# (operand has an MX format, its bit width, it has a group size) -> the route; None: the constructor refuses the combination
WEIGHT = {
    (True, 1, False): "mx", (True, 2, False): "mx", (True, 3, False): "mx", (True, 4, False): "mx", (True, 8, False): "mx", (True, 32, False): "mx",
    (False, 1, False): "low", (False, 2, False): "low",
    (False, 3, False): "sym", (False, 4, False): "sym", (False, 8, False): "sym",
    (False, 3, True): "group", (False, 4, True): "group", (False, 8, True): "group",
    (False, 32, False): "none",
    (False, 1, True): None, (False, 2, True): None, (False, 32, True): None,
    (True, 1, True): None, (True, 2, True): None, (True, 3, True): None, (True, 4, True): None, (True, 8, True): None, (True, 32, True): None,
}
ACT = {
    (True, 2, False): "mx", (True, 3, False): "mx", (True, 8, False): "mx", (True, 32, False): "mx",
    (False, 2, False): "none", (False, 32, False): "none",
    (False, 3, False): "row", (False, 8, False): "row",
    (False, 3, True): "group", (False, 8, True): "group",
    (False, 2, True): None, (False, 32, True): None,
    (True, 2, True): None, (True, 3, True): None, (True, 8, True): None, (True, 32, True): None,
}


def refusal(w_bits, a_bits, wl, al, wg, ag, wf, af, rot):
    """-> the ValueError text the constructor answers these arguments with (its checks in its order), or None"""
    if wf and (wg or wl):
        return "weight_format cannot be combined with weight_group_size or weight_layerwise"
    if af and (ag or al):
        return "act_format cannot be combined with act_group_size or act_layerwise"
    if rot and not (wf and af):
        return "mx_rotate needs both operands in an MX format (weight_format and act_format): (x R)(W R)^T = x W^T only when both are rotated"
    if wg and not 3 <= w_bits < 32:
        return f"weight_group_size applies to SymQuantizer weights (3 <= w_bits < 32), this layer has w_bits={w_bits}"
    if wg and wl:
        return "group_size cannot be combined with layerwise=True"
    if ag and not 2 < a_bits < 32:
        return f"act_group_size applies to quantized activations (2 < a_bits < 32), this layer has a_bits={a_bits}"
    if ag and al:
        return "group_size cannot be combined with layerwise=True"
    return None


@pytest.fixture()
def recorded(monkeypatch):
    """the launch callables of the three appliers as recorders: -> the list of (tag, tensor, extra) they were called with"""
    from llm_qat_amd import utils_quant as U
    calls = []

    def rec(tag, which, extra=None):
        def f(*args, **kw):
            calls.append((tag, args[which], None if extra is None else args[extra]))
            return args[which]
        return f

    class Fn:
        def __init__(self, tag):
            self.apply = rec(tag, 0)

    monkeypatch.setattr(U, "_mx_apply", rec("mx", 0, 2))                    # (x, fmt, rotate, rule, ste)
    monkeypatch.setattr(U, "_GroupQuantizer", Fn("group"))
    monkeypatch.setattr(U, "_SymQuantizerWeight", Fn("sym"))
    monkeypatch.setattr(U, "_SymQuantizerOperand", Fn("row"))
    monkeypatch.setattr(U.AsymQuantizer, "apply", staticmethod(rec("row", 0)))
    monkeypatch.setattr(U, "_shared_activation", rec("row", 1))            # (quantizer, x, bits, layerwise)
    monkeypatch.setattr(U.QuantizeLinear, "_quantized_weight", lambda self: calls.append(("sym", self.weight, None)) or self.weight)
    monkeypatch.setattr(U.QuantizeLinear, "_low_bit_weight", lambda self, w: calls.append(("low", w, None)) or w)
    monkeypatch.setattr(U.compiled, "fake_quant", lambda kind, x, clip, bits, layerwise, narrow=False: calls.append(("fq", x, None)) or x)
    monkeypatch.setattr(U.compiled, "low_bit_weight_op", lambda w, sc, bits: calls.append(("low", w, None)) or w)
    return calls


@pytest.mark.parametrize("a_bits", [2, 3, 8, 32])
@pytest.mark.parametrize("w_bits", [1, 2, 3, 4, 8, 32])
def test_one_decision_per_operand_and_three_appliers_of_it(recorded, w_bits, a_bits):
    from llm_qat_amd import utils_quant as U
    x = torch.randn(3, 64)
    accepted = 0
    for symmetric, wl, al, wg, ag, wf, af, rot in itertools.product((True, False), (False, True), (False, True), (None, 32), (None, 32),
                                                                    (None, "mxfp4"), (None, "mxfp4"), (False, True)):
        kw = dict(symmetric=symmetric, w_bits=w_bits, a_bits=a_bits, weight_layerwise=wl, act_layerwise=al, weight_group_size=wg,
                  act_group_size=ag, weight_format=wf, act_format=af, mx_rotate=rot)
        why = refusal(w_bits, a_bits, wl, al, wg, ag, wf, af, rot)
        if why is not None:
            with pytest.raises(ValueError) as e:
                U.QuantizeLinear(64, 8, **kw)
            assert str(e.value) == why, kw
            continue
        accepted += 1
        want_w, want_a = WEIGHT[wf is not None, w_bits, wg is not None], ACT[af is not None, a_bits, ag is not None]
        assert want_w is not None and want_a is not None, kw
        m = U.QuantizeLinear(64, 8, **kw)
        assert (m._weight_route(), m._act_route()) == (want_w, want_a), kw
        want = sorted((op, tag) for op, tag in (("w", want_w), ("a", want_a)) if tag != "none")
        paths = [("forward", m.forward), ("compiled", m._forward_compiled)] + ([("mx", m._forward_mx)] if wf or af else [])
        for path, fn in paths:
            del recorded[:]
            out = fn(x)
            assert out.shape == (3, 8)
            got = []
            for tag, t, rotate in recorded:
                op = "w" if t.data_ptr() == m.weight.data_ptr() else "a"
                if tag == "fq":     # the compiled path's one custom op: grouped operands reach it as the [-1, group] view
                    tag = "group" if t.shape[-1] == 32 else ("sym" if op == "w" else "row")
                if tag == "mx":
                    assert rotate is rot, (path, kw)
                got.append((op, tag))
            assert sorted(got) == want, (path, kw, got)
    assert accepted       # (every pair of bit widths has layers the constructor accepts)


# The one state in which the three ladders never agreed: a weight group size ASSIGNED to a 1-/2-bit layer (the constructor refuses one, so
# the cross above cannot reach it).  `_forward_mx` tested the group size before the bit width, the other two the bit width first; each
# path keeps its answer.  (path, w_bits) -> the weight's route
ASSIGNED_GROUP_ON_LOW_BITS = {
    ("forward", 1): "low", ("forward", 2): "low",
    ("compiled", 1): "low", ("compiled", 2): "low",
    ("mx", 1): "group", ("mx", 2): "group",
}


@pytest.mark.parametrize("w_bits", [1, 2])
def test_an_assigned_group_size_on_low_bits_keeps_each_paths_answer(recorded, w_bits):
    from llm_qat_amd import utils_quant as U
    x = torch.randn(3, 64)
    for act_format in (None, "mxfp4"):
        m = U.QuantizeLinear(64, 8, w_bits=w_bits, a_bits=8, act_format=act_format)
        m.weight_group_size = 32
        assert m._weight_route() == "low"
        paths = [("compiled", m._forward_compiled)] + ([("forward", m.forward)] if act_format is None else [("mx", m._forward_mx), ("mx", m.forward)])
        for path, fn in paths:
            del recorded[:]
            fn(x)
            got = [tag for tag, t, _ in recorded if t.data_ptr() == m.weight.data_ptr()]
            assert got == [ASSIGNED_GROUP_ON_LOW_BITS[path, w_bits]], (path, act_format, got)
