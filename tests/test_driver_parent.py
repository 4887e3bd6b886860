"""The twelve drivers of the single-pump, multi-channel and multi-line models against tests/golden/driver_parent.json.gz: what
they handed to the eight host functions of _native and what they returned or raised at the commit before they shared one driver
path, byte for byte.  Over the stand-in of tests/golden/driver_parent_cases.py: no GPU, no library."""
import gzip
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import driver_parent_cases as DC  # noqa: E402
import psa_amd  # noqa: E402

P = DC.package(psa_amd)
CASES = DC.cases(P)


@pytest.fixture(scope="module")
def record():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "driver_parent.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


def test_the_record_holds_exactly_the_cases(record):
    assert set(record) == set(CASES)
    assert len(CASES) > 400 and sum(not k.startswith("err/") for k in CASES) > 90


def test_every_case_is_the_parents_byte_for_byte(record):
    """Arrays are compared as dtype, shape and bytes and floats as their hex text, so a NaN equals itself, -0.0 is not +0.0
    and nothing has a tolerance; the calls are compared in the order one device saw them."""
    wrong = []
    for key, case in CASES.items():
        got = json.loads(json.dumps(DC.run_case(P, case)))
        want = record[key]
        if got != want:
            what = [k for k in ("raised", "returned", "calls") if got.get(k) != want.get(k)]
            wrong.append(f"{key}: {what}: {got.get('raised')} / {want.get('raised')}")
    assert not wrong, "\n".join(wrong)
