"""Both chain families against what the library returned before they shared one host path: every array
of every case of tests/golden/chain_parent_cases.py, compared with tests/golden/chain_parent.npz (recorded by
tests/golden/gen_golden_chain_parent.py on the parent commit's build) by its raw bytes -- NaNs equal, -0 != +0, no
tolerance."""
import os
import sys

import numpy as np
import pytest

import psa_amd._native as nat
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import chain_parent_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return CC.unpack(np.load(os.path.join(GOLDEN, "chain_parent.npz"), allow_pickle=False))


def test_the_record_holds_every_case_and_nothing_else(parent):
    want = {CC.key(fam, prec, name, N, f) for fam, prec, name, N in CC.cases() for f in CC.expected_fields(fam, name)}
    assert set(parent) == want


@pytest.mark.parametrize("fam,prec", CC.FAMILIES, ids=["-".join(f) for f in CC.FAMILIES])
def test_every_array_equals_the_parent_record_byte_for_byte(parent, fam, prec):
    n = 0
    for f, p, name, N in CC.cases():
        if (f, p) != (fam, prec):
            continue
        got = CC.run(nat, fam, prec, name, N)
        assert tuple(sorted(got)) == tuple(sorted(CC.expected_fields(fam, name))), (name, N)
        for field, a in got.items():
            ref = parent[CC.key(fam, prec, name, N, field)]
            a = np.ascontiguousarray(a)
            assert a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes(), (name, N, field)
        n += 1
    assert n
