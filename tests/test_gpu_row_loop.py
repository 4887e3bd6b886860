"""The row-driven z-loop of the fused float64 4-wave summary kernels: blocks of save_every steps in
4-, 2- and 1-step trips, straight-line row work, the exact test thinned to one per group of rows.

Three yardsticks, all bit for bit:
  (a) the TRAJECTORY launch of the same inputs, which keeps the event loop: A[-1] is its last saved row, and its own
      p_end (|A_sig|^2 of that row, formed in the step's frame), p_max (the NaN-propagating maximum over its rows) and
      first_bad_step are the summary launch's;
  (b) what the library built from the commit before this loop returned for the same grid (tests/golden/row_loop_parent.npz,
      recorded by tests/golden/gen_golden_row_loop.py);
  (c) failing points: first_bad_step against the oracle's per-step index and the save_every = 1 trajectory run, whose
      per-row test is a per-step test, in the mirrored and in the general loop.
The grid (tests/golden/row_loop_cases.py): N = 67 and 131; all lanes mirrored, or one asymmetric lane per wave; eleven
(n_steps, save_every) over every remainder of the 4-step trip, tails, several rows per test group, one, and groups longer
than 64 steps; check_nan off / block / exact; lossy and lossless; with and without the per-wave summary; 64- and 256-thread
workgroups."""
import os
import sys

import numpy as np
import pytest

import psa_amd._native as nat
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import row_loop_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu


def same(a, b) -> bool:
    """equal bits (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def parent():
    return RC.unpack(np.load(os.path.join(GOLDEN, "row_loop_parent.npz"), allow_pickle=False))


@pytest.mark.parametrize("N", RC.SIZES)
@pytest.mark.parametrize("which", RC.SETS)
@pytest.mark.parametrize("n_steps,se", RC.STEPS)
def test_summary_launch_against_trajectory_launch_and_parent_record(parent, n_steps, se, which, N):
    n_rows = n_steps // se
    for check in RC.CHECKS:
        for lossy in RC.LOSSY:
            tr = RC.run(nat, which, N, n_steps, se, check, lossy, traj=True)
            assert tr["traj"].shape == (N, n_rows + 1, 4)
            for wsum, block in RC.LAYOUTS:
                tag = (check, lossy, wsum, block)
                got = RC.run(nat, which, N, n_steps, se, check, lossy, wsum, block)
                # (a) the trajectory launch of the same inputs
                assert same(got["a_end"], tr["traj"][:, n_rows, :]), tag
                assert same(got["a_end"], tr["a_end"]), tag
                assert same(got["p_end"], tr["p_end"]), tag
                assert same(got["p_max"], tr["p_max"]), tag
                assert same(got["first_bad_step"], tr["first_bad_step"]), tag
                assert np.isfinite(got["p_max"]).all() and (got["first_bad_step"] == -1).all(), tag
                # (b) the parent commit's build
                for f in RC.FIELDS + (RC.WAVE_FIELDS if wsum else ()):
                    assert same(got[f], parent[RC.key(which, n_steps, se, check, lossy, wsum, block, f)][:N]), tag + (f,)
                if wsum:   # the signal's columns are the gain summary's
                    assert same(got["p_wave_end"][:, 2], got["p_end"]) and same(got["p_wave_max"][:, 2], got["p_max"]), tag


# ---- (c) failing points -----------------------------------------------------------------------------------------------
# Golden G9's blow-up (gamma = 12, dbeta = 0.01, dz = 0.1, p_in = (0.5, 0.5, 1e-5, 1e-5): past the stability edge of RK4 at
# once) made to fail at a chosen step: the powers scaled down by exp(ALPHA * dz * t) and given the gain -ALPHA, so that the
# point grows back to the edge after about t steps.  The oracle's first_bad_step is a staircase in t, one step per unit, each
# stair about twenty samples of the scan wide; a target takes the sample in the middle of its stair, 20 % in power from both
# edges (implementations differ by 1e-12).
ALPHA = -4.0
G9_GAMMA, G9_DBETA, G9_P_IN = 12.0, 0.01, np.array([0.5, 0.5, 1e-5, 1e-5])
FAIL_STEPS = ((205, 10), (64, 7), (140, 7), (200, 64), (250, 100))   # 6 rows per group | 9 | 9 | 1 | 1, blocks longer than 64 steps


def _scaled(t):
    return np.sqrt(G9_P_IN[None, :] * np.exp(ALPHA * RC.DZ * np.asarray(t, float))[:, None]).astype(complex)


@pytest.fixture(scope="module")
def stairs(oracle):
    """t of the middle of the stair of every first_bad_step the scan reaches (250 steps: every case below)"""
    t = np.linspace(0.0, 260.0, 5201)
    fb = oracle.sweep(np.full(t.size, G9_DBETA), z_max=250 * RC.DZ, n=250, save_every=10, gamma=G9_GAMMA, alpha=ALPHA,
                      a0=_scaled(t))["first_bad_step"]
    return {int(s): float(np.median(t[fb == s])) for s in np.unique(fb) if s >= 0 and (fb == s).sum() >= 15}


def _targets(n_steps, se):
    """first_bad_step in the first, a middle and the last row of a test group, on both sides of a group boundary and of a
    row, around the last saved row and in the tail"""
    rows_per_group = max(1, 64 // se)
    group = rows_per_group * se
    last_saved = n_steps // se * se
    want = {2, se - 2, se - 1, se, group // 2, group - se // 2, group - 1, group, group + 1, group + se + 1, 2 * group - 1, 2 * group,
            last_saved - 1, last_saved, last_saved + 1, n_steps - 2, n_steps - 1}
    return sorted(s for s in want if 2 <= s < n_steps)


@pytest.mark.parametrize("which", RC.SETS)
@pytest.mark.parametrize("n_steps,se", FAIL_STEPS)
def test_first_bad_step_of_failing_points(oracle, stairs, n_steps, se, which):
    targets = _targets(n_steps, se)
    assert all(s in stairs for s in targets), [s for s in targets if s not in stairs]
    N = 131
    t = np.full(N, 600.0)                         # never fails: 1e-104 of the edge's power, 1e-61 after 250 steps
    lanes = [k for k in range(N) if k % 3 == 1 and k not in RC.ASYM_LANES][:len(targets)]
    assert len(lanes) == len(targets)
    t[lanes] = [stairs[s] for s in targets]
    a0 = _scaled(t)
    if which == "asym":                           # unequal pumps in one lane of every wave: the general loop
        a0[list(RC.ASYM_LANES), 1] *= 0.9
    db = np.full(N, G9_DBETA)
    kw = dict(n_steps=n_steps, z_max=n_steps * RC.DZ, gamma=G9_GAMMA, alpha=ALPHA, a0=a0, extra_flags=nat.OPT_ONE_LANE)
    ref = oracle.sweep(db, z_max=n_steps * RC.DZ, n=n_steps, save_every=se, gamma=G9_GAMMA, alpha=ALPHA, a0=a0)
    assert list(ref["first_bad_step"][lanes]) == targets
    assert ((ref["first_bad_step"] >= 0).sum()) == len(targets)
    every = nat.sweep_host(db, save_every=1, exact_step=True, want_traj=True, **kw)
    for wsum in (False, True):
        got = nat.sweep_host(db, save_every=se, exact_step=True, wave_summary=wsum, **kw)
        assert np.array_equal(got["first_bad_step"], ref["first_bad_step"]), wsum
        assert np.array_equal(got["first_bad_step"], every["first_bad_step"]), wsum
        blk = nat.sweep_host(db, save_every=se, exact_step=False, wave_summary=wsum, **kw)
        exact = np.asarray(targets)
        last_saved = n_steps // se * se
        assert np.array_equal(blk["first_bad_step"][lanes], np.where(exact < last_saved, exact // se * se + se - 1, n_steps - 1))
        ok = ref["first_bad_step"] < 0
        assert same(got["a_end"][ok], blk["a_end"][ok]) and same(got["p_max"][ok], blk["p_max"][ok])
        if last_saved:
            assert same(got["a_end"][ok], every["traj"][ok, last_saved, :])
    if which == "asym":                           # the same index in both loops
        a0m = _scaled(t)
        mir = nat.sweep_host(db, save_every=se, exact_step=True, **dict(kw, a0=a0m))
        assert list(mir["first_bad_step"][lanes]) == targets
