"""Records tests/golden/abi_refusals.json: what every launching entry point of the C ABI refuses and how, as the library named by
LLMQAT_AMD_LIB answers the calls of tests/abi_refusal_cases.py.  The committed transcript comes from the library of the commit BEFORE
the host launch layer was refactored (a checkout of that commit, `python llm-qat_amd/build.py --out=<lib>`), so that the test replaying it
(tests/test_abi_refusals_cpu.py) pins every refusal's code, text and place in the order of checks across the refactor.

    LLMQAT_AMD_LIB=<lib built from the commit to record> python tests/golden/make_abi_refusals.py

No GPU: every call is refused (or finds an empty shape) before any launch, and the script asserts that while recording."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import abi_refusal_cases as R  # noqa: E402
from llm_qat_amd import _lib  # noqa: E402


def main():
    """The file holds every distinct (code, message) once, in `refusals`; `seeded` and `hand` point into that table."""
    assert os.environ.get("LLMQAT_AMD_LIB"), "name the library to record with LLMQAT_AMD_LIB"
    L = _lib.lib()
    lines = R.seeded_lines(_lib, L)
    assert list(lines) == R.launching(_lib)
    hand = []
    for what, name, args in R.hand(_lib):
        rc, msg = R.call(L, name, args)
        assert rc not in (0, R.ERR_LAUNCH) and msg, (what, name, rc, msg)      # refused, before any launch
        hand.append((what, name, (rc, msg)))
    table = sorted(set().union(*(R.pairs_of(ls) for ls in lines.values())) | {h[2] for h in hand})
    assert all(rc != R.ERR_LAUNCH for rc, _ in table)
    at = {p: i for i, p in enumerate(table)}
    row = json.dumps
    out = os.path.join(HERE, "abi_refusals.json")
    with open(out, "w") as f:      # one line per refusal, entry point and hand-written call
        f.write('{"recorded_from": %s, "seed": 0, "calls_per_entry_point": 400,\n "refusals": [\n' % row(L.fq_build_info().decode()))
        f.write(",\n".join("  " + row(list(p)) for p in table))
        f.write('\n ],\n "seeded": {\n')
        f.write(",\n".join("  %s: %s" % (row(n), row({"pairs": sorted(at[p] for p in R.pairs_of(ls)), "sha256": R.digest(ls)})) for n, ls in lines.items()))
        f.write('\n },\n "hand": [\n')
        f.write(",\n".join("  " + row([what, name, at[p]]) for what, name, p in hand))
        f.write("\n ]\n}\n")
    json.load(open(out))
    print(out, len(lines), "entry points,", len(table), "distinct refusals,", len(hand), "hand-written calls")


if __name__ == "__main__":
    main()
