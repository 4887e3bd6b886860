"""The multi-channel, single-pump and multi-line sweeps against what the library returned before they shared one host path
(DESIGN.md 3.5f): every array of every case of tests/golden/wave_family_parent_cases.py -- the host wrappers, the `_dev` entry
points on torch buffers and a two-span chain of the pairs and of the comb -- compared with
tests/golden/wave_family_parent.npz (recorded by tests/golden/gen_golden_wave_family_parent.py on the parent commit's build)
by its raw bytes: NaNs equal, -0 != +0, no tolerance."""
import os
import sys

import numpy as np
import pytest

import psa_amd._native as nat
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import wave_family_parent_cases as WC  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = ["-".join(g) for g in WC.GROUPS]


@pytest.fixture(scope="module")
def parent():
    return WC.unpack(np.load(os.path.join(GOLDEN, "wave_family_parent.npz"), allow_pickle=False))


def same_bytes(got: dict, parent: dict, key_of, fields, what):
    assert tuple(sorted(got)) == tuple(sorted(fields)), what
    for field, a in got.items():
        ref = parent[key_of(field)]
        a = np.ascontiguousarray(a)
        assert a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes(), (what, field)


def test_the_record_holds_every_case_and_nothing_else(parent):
    assert set(parent) == WC.expected_keys()


@pytest.mark.parametrize("group,prec", WC.GROUPS, ids=IDS)
def test_every_host_array_equals_the_parent_record_byte_for_byte(parent, group, prec):
    n = 0
    for fam, p, name, N, rows in WC.cases():
        if (WC.group_of(fam), p) != (group, prec):
            continue
        got = WC.run(nat, fam, prec, name, N, rows)
        same_bytes(got, parent, lambda f: WC.key(fam, prec, name, N, rows, f), WC.FIELDS + (("traj",) if rows else ()),
                   (fam, name, N, rows))
        n += 1
    assert n


@pytest.mark.parametrize("fam,prec", WC.DEV, ids=["-".join(d) for d in WC.DEV])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "traj_ld"])
def test_the_dev_entry_points_equal_the_parent_record_byte_for_byte(parent, fam, prec, padded):
    torch = pytest.importorskip("torch")
    got = WC.run_dev(nat, torch, fam, prec, padded)
    same_bytes(got, parent, lambda f: WC.dev_key(fam, prec, padded, f), WC.FIELDS + (("traj",) if padded else ()), (fam, prec, padded))


@pytest.mark.parametrize("fam", WC.CHAINS)
def test_a_two_span_chain_equals_the_parent_record_byte_for_byte(parent, fam):
    same_bytes(WC.run_chain(nat, fam), parent, lambda f: WC.chain_key(fam, f), WC.FIELDS + ("traj",), fam)
