"""Every sweep-family entry point answers a table of invalid calls exactly as tests/golden/cabi_errors.json records: the same
return code and the same psa_last_error() text, rule by rule, with two rules broken at once to pin their order, and the empty
(n_points == 0) calls that return 0.  The table and its recorder are tests/golden/gen_golden_cabi_errors.py; every call carries
dummy host pointers and is rejected before any device call, so this runs without a GPU."""
import importlib.util
import json
import os

import pytest

import psa_amd._native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_cabi_errors", os.path.join(GOLDEN, "gen_golden_cabi_errors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.OUT, encoding="utf-8") as _f:
    RECORDED = json.load(_f)
SYMBOLS = sorted(gen.cases())


def test_the_table_covers_every_sweep_family_entry_point_on_both_faces():
    families = [s for s in nat.EXPORTED_SYMBOLS if s.startswith(("psa_rk4_", "psa_rk45_")) and not s.endswith("_workspace_bytes")]
    assert sorted(families) == SYMBOLS and len(SYMBOLS) == 30
    ids = {f"{s}:{case}" for s in SYMBOLS for case in gen.cases()[s][1]}
    assert ids == set(RECORDED)                                   # nothing recorded is skipped, nothing replayed is unrecorded
    for s in SYMBOLS:
        mine = [k for k in RECORDED if k.startswith(s + ":")]
        assert sum(":two:" in k for k in mine) >= 1 and sum(RECORDED[k][0] == 0 for k in mine) >= 1, s
    assert all(rc < 0 and rc != -7 and msg for rc, msg in RECORDED.values() if rc != 0)   # argument errors: no device was asked for


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_invalid_calls_get_the_recorded_code_and_message(symbol):
    got = gen.replay(nat.lib(), symbol)
    want = {k: v for k, v in RECORDED.items() if k.startswith(symbol + ":")}
    assert got == want
