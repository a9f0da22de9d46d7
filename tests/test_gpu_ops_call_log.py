"""GPU tier: ops.py's masked STE backwards (train_backward, train_backward_wide, pair_backward, pair_backward_wide, multi_backward,
ste_backward_mask) and N-tensor Sym forwards (pair_forward, multi_forward) call the C ABI, allocate, return, fall back and raise exactly as
the recording in ops_call_log.json says -- which was taken at commit a8f632c, before their per-tensor work moved into ops._mask_slot
(ops_call_cases.py: the cases, the recorder and what a log holds)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ops_call_cases as C  # noqa: E402


def canon(v):
    """type-strict form: -2 and -2.0 are different cells"""
    return json.dumps(v, sort_keys=True)


def test_call_log_equals_the_recording():
    with open(C.LOG) as f:
        want = json.load(f)
    got = C.record()
    unresolved = [name for name, log in got.items() if '"?' in canon(log["calls"])]
    assert not unresolved, f"pointers that are neither an input, a result nor a known temporary: {unresolved}"
    assert list(got) == list(want), f"cases differ: {sorted(set(got) ^ set(want))}"
    bad = {}
    for name in want:
        if canon(got[name]) != canon(want[name]):
            bad[name] = [(k, got[name][k], want[name][k]) for k in want[name] if canon(got[name].get(k)) != canon(want[name][k])]
    assert not bad, f"{len(bad)} of {len(want)} cases differ from the recording (cell, got, recorded); the first: {next(iter(bad.items()))}"


def test_every_case_family_is_recorded_and_nothing_ineligible_launches():
    with open(C.LOG) as f:
        want = json.load(f)
    assert [name for name, _ in C.cases()] == list(want)
    for name, log in want.items():
        if "/ineligible/" in name:
            assert log["calls"] == [] and log["returns"] is None and log["raises"] is None, name
    called = {c[0] for log in want.values() for c in log["calls"]}
    assert called >= {"fq_sym_fwd_pair", "fq_sym_fwd_multi", "fq_sym_fwd_multi_v", "fq_ste_bwd_mask", "fq_ste_bwd_mask_pair",
                      "fq_ste_bwd_mask_wide", "fq_ste_bwd_mask_multi", "fq_ste_bwd_mask_multi_v"}, called
