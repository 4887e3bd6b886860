"""``chain`` and ``direct`` of the three NumPy chain restatements against tests/golden/chain_twin_parent.json: every array they
returned, for the cases of tests/golden/chain_twin_parent_cases.py, at the commit before they shared the span loop of
tests/chain_np.py, as dtype, shape and the SHA-256 of the bytes.  NumPy alone: no GPU, no library."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import chain_twin_parent_cases as TC  # noqa: E402

CASES = TC.cases()


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(ROOT, "tests", "golden", "chain_twin_parent.json")) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_cases(record):
    assert set(record) == set(CASES)
    for name, twin in TC.TWINS.items():
        assert sum(key.startswith(name) and "/chain/" in key for key in CASES) >= 4 * len(TC.WIDTHS[name])
        assert any(key.startswith(name) and "/direct/" in key for key in CASES)
        for special in ("failing", "closed_form"):
            assert hasattr(twin, special + "_case") == (f"{name}/{special}/chain" in " ".join(CASES)), (name, special)


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_twin_returns_the_parents_bytes(record, key):
    assert TC.run_case(CASES[key]) == record[key]
