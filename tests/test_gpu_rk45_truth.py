"""The adaptive (RK45) sweep kernel against the 80-bit yardstick of its own discrete scheme (tests/truth_rk45_ld.py), through
nat.rk45_sweep_host.

tests/test_gpu_rk45.py holds the kernel within 1e-10 of a float64 twin that itself sits 1e-15..2e-13 from the yardstick: three
to five decimal digits in which the kernel can get worse unseen.  Here kernel and twin are measured against Dormand-Prince 5(4)
with scipy's controller in 80 bits, which takes the twin's accepted and rejected attempts at every point of every set
(tests/test_truth_rk45_host.py asserts it), so that the truncation error cancels as it does on a fixed grid.  At the points
where the kernel's counts equal the yardstick's the bar of tests/test_gpu_truth.py applies to a_end, p_end, p_max and the rows,

    median(e_gpu) <= 4 median(e_twin)   and   max(e_gpu) <= 8 max(e_twin)

over those points, with NO floor: the kernel carries no phase -- an exact sincos at every stage -- and two plain float64
statements of the scheme meet this bar against each other without one (TC.FLOOR_RK45).  The 1e-10 against the twin stays
beside it.  At most 3 of the 67 points, the 5 % tests/test_gpu_rk45.py grants, may take other counts (the last bits of an error
norm near 1 decide an attempt); each of them is printed and held to 100 rtol of the yardstick.  Points that end with status 1
or 2 are not in these sets: the G9 fixtures and test_failure_statuses_and_gain keep them.

Inputs and the cached 80-bit runs: tests/truth_cases.py.  Each case prints one line of the record (profiles/truth_errors.txt)."""
import numpy as np
import pytest

import truth_cases as TC
import truth_ld as T
from test_gpu_truth import meets_the_bar          # raises BarMissed, as in every case of the suite

import psa_amd._native as nat

pytestmark = pytest.mark.gpu

MAY_DIFFER = 3                         # of 67 points: 5 %

# every set with its rows, and the lossy set once more without: the no-rows instantiation of the kernel
CASES = [(name, True) for name in TC.RK45_SETS] + [("lossy-r9", False)]


def launch(inputs, rows):
    return nat.rk45_sweep_host(inputs["dbeta"], dbeta2=inputs.get("dbeta2"), gamma=inputs["gamma"], alpha=inputs["alpha"],
                               a0=inputs["a0"], n_out=inputs["n_out"] if rows else 0, **TC.rk45_tolerances(inputs))


def against_the_twin(got, twin):
    """Per point, of the point's largest wave: a_end and the rows, and wave 2's p_end / p_max as moduli."""
    top = np.max(np.abs(twin["a_end"]), axis=1)
    out = dict(a_end=T.point_err(got["a_end"], twin["a_end"]))
    for k in ("p_end", "p_max"):
        out[k] = np.abs(np.sqrt(got[k]) - np.sqrt(twin[k])) / top
    if got["rows"] is not None:
        out["rows"] = T.point_err(got["rows"], twin["rows"])
    return out


@pytest.mark.parametrize("name,rows", CASES, ids=[n + ("" if r else "-no-rows") for n, r in CASES])
def test_rk45_against_the_yardstick(name, rows):
    inputs = TC.rk45(name)
    truth, twin = inputs["truth"], inputs["twin"]
    got = launch(inputs, rows)
    case = name + ("" if rows else "-no-rows")

    # every point
    assert np.all(got["status"] == 0)
    np.testing.assert_array_equal(got["z_end"], np.full(TC.N, inputs["z_max"]))
    if rows:
        assert got["traj"].shape == truth["rows"].shape
        np.testing.assert_array_equal(got["traj"][:, 0], inputs["a0"])
        assert np.max(T.point_err(got["traj"][:, -1], got["a_end"])) < 1e-13
    else:
        assert got["traj"] is None

    # the points that took other attempts than the yardstick: few, finished, within the project's bound, on record
    same = TC.rk45_same_steps(got, truth)
    formed = TC.rk45_form(got, rows)
    e_all = TC.errors(formed, truth)
    for i in np.nonzero(~same)[0]:
        print(f"\ntruth | rk45 | {case} | point {i} takes {got['n_accepted'][i]} + {got['n_rejected'][i]} attempts, the yardstick "
              f"{truth['n_accepted'][i]} + {truth['n_rejected'][i]} | " + " ".join(f"{k} {v[i]:.2e}" for k, v in e_all.items()), end="")
    assert (~same).sum() <= MAY_DIFFER, (~same).sum()
    for k, v in e_all.items():
        assert np.all(v[~same] < 100 * inputs["rtol"]), (k, v[~same])

    # the points on the yardstick's steps: the bar, and the bound against the twin beside it
    g, t, w = TC.rk45_at(formed, same), TC.rk45_at(truth, same), TC.rk45_at(TC.rk45_form(twin, rows), same)
    missed = TC.judge("rk45", case, g, dict(truth=t, twin=w), TC.FLOOR_RK45)
    for k, v in against_the_twin(g, w).items():
        assert v.max() < TC.RK45_TWIN_RTOL, (k, v.max())
    meets_the_bar(missed)
