"""CPU tier: every refusal of the C ABI keeps its code, its text and its place in the order of checks.  tests/golden/abi_refusals.json
is a transcript recorded (tests/golden/make_abi_refusals.py) from the library as it was before the host launch layer moved behind shared
helpers; the calls (tests/abi_refusal_cases.py) are replayed against the library under test and compared with it.  Per entry point the
400 seeded calls of test_abi_and_host.py's fuzz give the set of distinct (code, message) pairs and a SHA-256 over the ordered
`code|message` lines; the hand-written calls, which reach the later checks with non-NULL pointers that are never dereferenced, are kept one
by one.  The file holds every distinct (code, message) once; the entry points and the hand-written calls point into that table.  Every call
is refused before any launch, so no kernel runs and no GPU is needed."""
import json
import os

import pytest

import abi_refusal_cases as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "abi_refusals.json")))


def test_seeded_calls_are_refused_as_recorded(golden):
    from llm_qat_amd import _lib
    got = R.seeded_lines(_lib, _lib.lib())
    want, table = golden["seeded"], [tuple(p) for p in golden["refusals"]]
    assert golden["seed"] == 0 and golden["calls_per_entry_point"] == 400 and len(set(table)) == len(table)
    assert sorted(got) == sorted(want) == sorted(R.launching(_lib))
    for name in R.launching(_lib):
        assert len(got[name]) == 400
        assert R.pairs_of(got[name]) == {table[i] for i in want[name]["pairs"]}, name
        assert all(rc != R.ERR_LAUNCH for rc, _ in R.pairs_of(got[name])), name
        assert R.digest(got[name]) == want[name]["sha256"], name         # the same refusal for the same call, in order


def test_hand_written_calls_are_refused_as_recorded(golden):
    from llm_qat_amd import _lib
    L = _lib.lib()
    calls = R.hand(_lib)
    table = [tuple(p) for p in golden["refusals"]]
    assert [(c[0], c[1]) for c in calls] == [(h[0], h[1]) for h in golden["hand"]]
    for (what, name, args), (_, _, i) in zip(calls, golden["hand"]):
        assert table[i][0] not in (0, R.ERR_LAUNCH)
        assert R.call(L, name, args) == table[i], (what, name)


def test_the_hand_written_list_reaches_the_later_checks(golden):
    """what the list is for: each of these refusals is in it, at the entry point that makes it"""
    texts = {golden["refusals"][i][1] for _, _, i in golden["hand"]}
    for part in ("in-place (y == x) is not supported", "a mask needs row_bounds_out too", "unknown bins container", "autocast arithmetic applies to",
                 "does not divide cols", "the kernel serves groups of 4..64", "unknown MX format code", "FP6 formats have no export packing",
                 "unknown flag bits", "rotation run", "mask_out must not alias x or y", "mask must not alias g or gx",
                 "in-place (gx == g) is not supported with the rotation", "is not a positive multiple of 128", "mask buffer too small: need 32 bytes",
                 "a single tensor goes first", "an in-place tensor (gx == g) needs equal views", "two-pass path needs", "exceed one launch's grid",
                 "pointers must be 16-byte aligned", "pair launch: rows must be 16-byte aligned"):
        assert any(part in m for m in texts), part
    assert {e for _, e, _ in golden["hand"]} >= {"fq_sym_fwd", "fq_sym_fwd_autocast", "fq_sym_export", "fq_asym_export", "fq_sym_row_scales", "fq_group_fwd",
                                                "fq_mx_fwd_ex", "fq_mx_export_ex", "fq_mx_ste_bwd", "fq_mx_gemm", "fq_ste_bwd_mask_wide", "fq_ste_bwd_mask_multi_v"}
