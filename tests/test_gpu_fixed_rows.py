"""The fixed-row form of the row-driven z-loop: launches of the fused float64 4-wave one-lane summary
kernel with save_every = 10 and at least one row run their saved rows as blocks of ten steps in straight line, in an
instantiation compiled for that stride; every other stride, and a launch too short for a row, keeps the run-time loop.

Nothing may depend on which loop ran the rows, so every comparison is bit for bit (NaN payloads and signed zeros included),
through the C-ABI with OPT_ONE_LANE:
  (a) the save_every = 1 TRAJECTORY launch of the same inputs (its own loop, one row per step): A[-1] is its row
      10 * n_rows and first_bad_step its index.  |A_sig|^2 of a row is formed in the step's frame and leaves the kernel as
      p_end only, so p_end at row 10 k is the p_end of the every-step launch ENDED at step 10 k (dz = 1/8: the step length
      is the same number whatever n_steps is, and the steps before the end do not know where the end is -- the fixture
      checks that too), and p_max is the NaN-propagating maximum of those over k, z = 0 included;
  (b) the save_every = 5 summary launch (the run-time loop) that ends on the same row: a_end, p_end, first_bad_step, and
      with the per-wave summary p_wave_end;
  (c) failing points, built as tests/test_gpu_row_loop.py builds them (G9's staircase): first_bad_step against the oracle
      and the save_every = 1 run, in the mirrored and in the general loop;
  (d) the dispatch's fallback: n_steps = 9 (no row) and save_every = 11 against their own trajectory launches.
tests/test_gpu_row_loop.py pins the same path to the bits recorded before it existed (its save_every = 10 cases)."""
import sys

import numpy as np
import pytest

import psa_amd._native as nat
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import row_loop_cases as RC  # noqa: E402
import test_gpu_row_loop as RL  # noqa: E402
from test_gpu_row_loop import same, stairs  # noqa: E402,F401  (stairs: the module's fixture, used below)

pytestmark = pytest.mark.gpu

ROW = 10
DZ = 0.125                                     # a power of two: n * DZ / n == DZ exactly, for every n
# one row | a tail of 5 | exactly one test group of 6 rows | one row past a group | many groups plus a tail
N_STEPS = (10, 20, 25, 60, 70, 205)
K_MAX = max(N_STEPS) // ROW


def launch(which, N, n_steps, se, check="off", lossy=True, wsum=False, block=256, traj=False):
    """RC.run at dz = 1/8"""
    db, gam, a0 = RC.points(which)
    flags = nat.OPT_ONE_LANE | (nat.OPT_BLOCK64 if block == 64 else 0)
    return nat.sweep_host(db[:N], n_steps=n_steps, z_max=n_steps * DZ, save_every=se, gamma=gam[:N],
                          alpha=1.15e-2 if lossy else 0.0, a0=a0[:N], extra_flags=flags, wave_summary=wsum, want_traj=traj,
                          **RC.check_kw(check))


@pytest.fixture(scope="module")
def every_step():
    """(which, lossy) -> the save_every = 1 trajectory launch of all 131 points over the longest case, and p_end of that
    launch ended at step 10 k, k = 0 .. K_MAX (k = 0: |A_sig(0)|^2, from a launch without a row).  Computed once."""
    ref = {}
    for which in RC.SETS:
        for lossy in RC.LOSSY:
            full = launch(which, RC.N_ALL, max(N_STEPS), 1, lossy=lossy, traj=True)
            p_rows = [launch(which, RC.N_ALL, 1, 2, lossy=lossy)["p_end"]]
            for k in range(1, K_MAX + 1):
                cut = launch(which, RC.N_ALL, ROW * k, 1, lossy=lossy, traj=True)
                assert same(cut["traj"], full["traj"][:, :ROW * k + 1, :]), (which, lossy, k)   # a prefix, bit for bit
                p_rows.append(cut["p_end"])
            assert np.isfinite(full["traj"].view(float)).all() and (full["first_bad_step"] == -1).all()
            ref[which, lossy] = dict(traj=full["traj"], p_rows=np.stack(p_rows))
    return ref


def nan_max(rows):
    """np.max over the saved rows as the kernels form it: a NaN row replaces the maximum"""
    pm = rows[0].copy()
    for pe in rows[1:]:
        pm = np.where((pe > pm) | (pe != pe), pe, pm)
    return pm


@pytest.mark.parametrize("N", RC.SIZES)
@pytest.mark.parametrize("which", RC.SETS)
@pytest.mark.parametrize("n_steps", N_STEPS)
def test_ten_step_rows_against_every_step_launch_and_stride_five(every_step, n_steps, which, N):
    n_rows = n_steps // ROW
    for lossy in RC.LOSSY:
        ref = every_step[which, lossy]
        p_end = ref["p_rows"][n_rows, :N]
        p_max = nan_max(ref["p_rows"][:n_rows + 1, :N])
        for check in RC.CHECKS:
            tr = launch(which, N, n_steps, 1, check, lossy, traj=True)           # (a) the same inputs, a row per step
            assert same(tr["traj"], ref["traj"][:N, :n_steps + 1, :]), (check, lossy)
            for wsum, block in RC.LAYOUTS:
                tag = (check, lossy, wsum, block)
                got = launch(which, N, n_steps, ROW, check, lossy, wsum, block)
                assert same(got["a_end"], tr["traj"][:, ROW * n_rows, :]), tag
                assert same(got["p_end"], p_end), tag
                assert same(got["p_max"], p_max), tag
                assert same(got["first_bad_step"], tr["first_bad_step"]) and (got["first_bad_step"] == -1).all(), tag
                # (b) the run-time loop at save_every = 5, ended on the same row (the tail of 5 would be a row there)
                five = launch(which, N, ROW * n_rows, 5, check, lossy, wsum, block)
                assert same(got["a_end"], five["a_end"]), tag
                assert same(got["p_end"], five["p_end"]), tag
                assert same(got["first_bad_step"], five["first_bad_step"]), tag
                if wsum:
                    assert same(got["p_wave_end"], five["p_wave_end"]), tag
                    assert same(got["p_wave_end"][:, 2], got["p_end"]) and same(got["p_wave_max"][:, 2], got["p_max"]), tag
                    assert (got["p_wave_max"] >= got["p_wave_end"]).all(), tag


# ---- (c) failing points: first_bad_step in the first, a middle and the last row of a test group (6 rows, 60 steps), on both
# sides of a group boundary, at the last saved row +-1 and in the tail
FAIL_TARGETS = {
    205: (2, 5, 9, 10, 30, 35, 55, 59, 60, 61, 71, 119, 120, 121, 199, 200, 201, 203, 204),
    70: (2, 9, 30, 59, 60, 61, 68, 69),          # one row past a group; 69 is the last saved row - 1
}


@pytest.mark.parametrize("which", RC.SETS)
@pytest.mark.parametrize("n_steps", sorted(FAIL_TARGETS))
def test_first_bad_step_of_failing_points(oracle, stairs, n_steps, which):  # noqa: F811
    targets = list(FAIL_TARGETS[n_steps])
    assert all(s in stairs for s in targets), [s for s in targets if s not in stairs]
    N = 131
    t = np.full(N, 600.0)                         # never fails (tests/test_gpu_row_loop.py)
    lanes = [k for k in range(N) if k % 3 == 1 and k not in RC.ASYM_LANES][:len(targets)]
    assert len(lanes) == len(targets)
    t[lanes] = [stairs[s] for s in targets]
    a0 = RL._scaled(t)
    if which == "asym":                           # unequal pumps in one lane of every wave: the general loop
        a0[list(RC.ASYM_LANES), 1] *= 0.9
    db = np.full(N, RL.G9_DBETA)
    kw = dict(n_steps=n_steps, z_max=n_steps * RC.DZ, gamma=RL.G9_GAMMA, alpha=RL.ALPHA, a0=a0, extra_flags=nat.OPT_ONE_LANE)
    ref = oracle.sweep(db, z_max=n_steps * RC.DZ, n=n_steps, save_every=ROW, gamma=RL.G9_GAMMA, alpha=RL.ALPHA, a0=a0)
    assert list(ref["first_bad_step"][lanes]) == targets
    assert ((ref["first_bad_step"] >= 0).sum()) == len(targets)
    every = nat.sweep_host(db, save_every=1, exact_step=True, want_traj=True, **kw)
    ok = ref["first_bad_step"] < 0
    last_saved = n_steps // ROW * ROW
    for wsum in (False, True):
        got = nat.sweep_host(db, save_every=ROW, exact_step=True, wave_summary=wsum, **kw)
        assert np.array_equal(got["first_bad_step"], ref["first_bad_step"]), wsum
        assert np.array_equal(got["first_bad_step"], every["first_bad_step"]), wsum
        blk = nat.sweep_host(db, save_every=ROW, exact_step=False, wave_summary=wsum, **kw)
        exact = np.asarray(targets)
        assert np.array_equal(blk["first_bad_step"][lanes], np.where(exact < last_saved, exact // ROW * ROW + ROW - 1, n_steps - 1))
        assert same(got["a_end"][ok], blk["a_end"][ok]) and same(got["p_max"][ok], blk["p_max"][ok])
        assert same(got["a_end"][ok], every["traj"][ok, last_saved, :])
    if which == "asym":                           # the same index in both loops
        mir = nat.sweep_host(db, save_every=ROW, exact_step=True, **dict(kw, a0=RL._scaled(t)))
        assert list(mir["first_bad_step"][lanes]) == targets


# ---- (d) what the dispatch leaves on the run-time loop
@pytest.mark.parametrize("which", RC.SETS)
@pytest.mark.parametrize("n_steps,se", ((9, 10), (25, 11), (205, 11)))
def test_launches_the_fixed_row_form_does_not_take(n_steps, se, which):
    n_rows = n_steps // se
    for check in RC.CHECKS:
        for lossy in RC.LOSSY:
            tr = launch(which, 131, n_steps, se, check, lossy, traj=True)
            assert tr["traj"].shape == (131, n_rows + 1, 4)
            for wsum, block in RC.LAYOUTS:
                tag = (check, lossy, wsum, block)
                got = launch(which, 131, n_steps, se, check, lossy, wsum, block)
                assert same(got["a_end"], tr["traj"][:, n_rows, :]), tag
                for f in RC.FIELDS:
                    assert same(got[f], tr[f]), tag + (f,)
                assert np.isfinite(got["p_max"]).all() and (got["first_bad_step"] == -1).all(), tag
