"""The frame-anchored RK4 step of the float64 four-wave sweeps (tests/test_step_frame_identity.py
holds the host restatement).  The one-lane kernel's two z-loops and the two-lane kernel's mirrored path integrate the sidebands
in a frame that moves with the step and write the record through F(step) = exp(i*dbeta*(z_step + d)/2), seeded exactly at the
multiples of 64 steps and rotated once per step in between.  What can go wrong is at the edges of that: runs that end just
before, on and after a seed (63, 64, 65 steps; 333 = five seeds and a tail), a row that falls on a seed, no saved row at all,
a partial wave, both workgroup sizes, the every-step loop, and the summary kernels, which build F only where A[-1] is stored.

Measured on an MI355X (worst relative error on A[-1] against the oracle over every case of the first test, bar 1e-9):
2.5e-14 for |dbeta| <= 0.05 and 3.6e-13 for |dbeta| = 12 rad per step (both at 333 steps, 131 points).
The long case (64 points of the headline sweep, 1e5 steps): 1.28e-11 on A[-1] (signal 1.19e-11, pump 1.28e-11) and 8.2e-12
on the maximum of |A3|^2; the carried-phase step it replaces gave 9.7e-12 (3.6e-12, 9.7e-12) and 1.5e-12 on the same points
(profiles/step_frame.log)."""
import numpy as np
import pytest

import psa_amd._native as nat
from conftest import RTOL_F64, rel_err

pytestmark = pytest.mark.gpu

GAMMA = 0.0115
LANES = {"one": nat.OPT_ONE_LANE, "two": nat.OPT_SPLIT_POINT}
BLOCKS = {"wg256": 0, "wg64": nat.OPT_BLOCK64}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _inputs(N, mirrored, big, seed):
    """per-point amplitudes with phases; dbeta within +-0.05 at h = 0.1, or +-12 (a spread below it) at h = 1: 12 rad per step"""
    rng = np.random.default_rng(seed)
    amp = np.sqrt(rng.uniform([0.2, 0.2, 1e-6, 1e-6], [0.8, 0.8, 1e-3, 1e-3], (N, 4)))
    a0 = amp * np.exp(1j * rng.uniform(-3.1, 3.1, (N, 4)))
    if mirrored:
        a0[:, 1], a0[:, 3] = a0[:, 0], a0[:, 2]
    if big:
        db, h = np.where(np.arange(N) % 2 == 0, 12.0, -12.0) * rng.uniform(0.9, 1.0, N), 1.0
        db[0] = 12.0
    else:
        db, h = rng.uniform(-0.05, 0.05, N), 0.1
        db[0] = 0.05
    return db, h, a0, rng.uniform(5e-3, 2e-2, N), rng.uniform(5e-5, 3e-4, N)


@pytest.mark.parametrize("n", [63, 64, 65, 333])
@pytest.mark.parametrize("N", [131, 1])
def test_every_layout_and_stride_against_the_oracle_and_each_other(oracle, N, n):
    """Mirrored and asymmetric a0, dbeta within +-0.05 and at +-12, lossy and PSA_OPT_LOSSLESS, save_every 1 / 7 / 64 / 1000
    (1000: no saved row, A[-1] = a0), both workgroup sizes, one and two lanes per point.  Each combination: A[-1], |A3|^2 at
    the end and its maximum against the oracle at 1e-9; the summary launch's A[-1] equal IN BITS to the last row of the
    trajectory launch and to that row of the every-step trajectory; row 0 equal to a0 in bits."""
    worst = {False: 0.0, True: 0.0}
    for mirrored in (True, False):
        for big in (False, True):
            db, h, a0, gam, al = _inputs(N, mirrored, big, 1000 * n + N)
            for lossy in (True, False):
                alpha = al if lossy else 0.0
                base = dict(n_steps=n, z_max=h * n, gamma=gam, alpha=alpha, a0=a0)
                every = {}
                for se in (1, 7, 64, 1000):
                    ref = oracle.sweep(db, z_max=h * n, n=n, save_every=se, gamma=gam, alpha=alpha, a0=a0)
                    last = n // se * se
                    for lname, lanes in LANES.items():
                        for bname, block in BLOCKS.items():
                            tag = (mirrored, big, lossy, se, lname, bname)
                            flags = lanes | block | (0 if lossy else nat.OPT_LOSSLESS)
                            summ = nat.sweep_host(db, save_every=se, extra_flags=flags, **base)
                            traj = nat.sweep_host(db, save_every=se, extra_flags=flags, want_traj=True, **base)
                            err = rel_err(summ["a_end"], ref["a_end"])
                            print(f"{tag}: a_end rel err {err:.3e}")
                            worst[big] = max(worst[big], err)
                            assert err < RTOL_F64, tag
                            assert rel_err(summ["p_end"], ref["p_end"]) < RTOL_F64, tag
                            assert rel_err(summ["p_max"], ref["p_max"]) < RTOL_F64, tag
                            assert (summ["first_bad_step"] == -1).all() and (traj["first_bad_step"] == -1).all(), tag
                            assert same_bits(traj["traj"][:, 0, :], a0), tag
                            assert same_bits(summ["a_end"], traj["traj"][:, -1, :]), tag
                            for k in ("a_end", "p_end", "p_max"):
                                assert same_bits(summ[k], traj[k]), (tag, k)
                            if se == 1:
                                every[lname, bname] = traj["traj"]
                            else:       # the stride only selects rows
                                assert same_bits(traj["traj"], every[lname, bname][:, 0:last + 1:se, :]), tag
                            if last == 0:
                                assert same_bits(summ["a_end"], a0), tag
    print(f"N={N} n={n}: worst a_end rel err {worst[False]:.3e} (|dbeta| <= 0.05), {worst[True]:.3e} (|dbeta| = 12)")


@pytest.mark.parametrize("lname", list(LANES))
@pytest.mark.parametrize("se", [1, 7, 64])
def test_a_mirrored_wave_and_an_asymmetric_lane_agree_in_bits_with_a_trajectory(se, lname):
    """192 points: 64 mirrored ones, the same 64 with point 40's idler off, and the mirrored 64 again; 333 steps, rows
    requested, exact failure index.  One lane per point: the middle wave runs the general stage, which is the mirrored stage
    with duplicates -- equal bits in every other lane.  Two lanes per point: a wave holds 32 points; the wave of points 96..127
    runs the two-lane stage (products paired per lane: equal to rounding), points 64..95 are a mirrored wave again."""
    db64, h, a64, gam64, al64 = _inputs(64, True, False, 5)
    pick = np.r_[0:64, 0:64, 0:64]
    a0 = a64[pick].copy()
    a0[64 + 40, 3] = 1.5 * a0[64 + 40, 2]
    got = nat.sweep_host(db64[pick], n_steps=333, z_max=h * 333, save_every=se, gamma=gam64[pick], alpha=al64[pick], a0=a0,
                         want_traj=True, check_nan=True, exact_step=True, extra_flags=LANES[lname])
    assert (got["first_bad_step"] == -1).all()
    same = np.array([k for k in range(64) if k != 40]) if lname == "one" else np.arange(32)
    near = np.array([k for k in range(32, 64) if k != 40])
    for k in ("traj", "a_end", "p_end", "p_max"):
        v = got[k]
        assert same_bits(v[0:64], v[128:192]), k
        assert same_bits(v[same], v[64 + same]), k
        assert rel_err(v[64 + near], v[near]) < 1e-11, k
    assert same_bits(got["traj"][:, -1, :], got["a_end"])


@pytest.mark.parametrize("mirrored", [True, False])
@pytest.mark.parametrize("lname", list(LANES))
def test_the_replayed_first_bad_step_is_the_every_step_runs(mirrored, lname):
    """Forty of 131 points get a graded negative loss and blow up at steps spread over the run: the summary launch finds the
    index by replaying the failing block from its checkpoint (which no longer holds a phase factor), the every-step trajectory
    launch tests every row; both are the same forward pass, so the indices must be equal, whatever the stride."""
    N, n = 131, 333
    db, h, a0, gam, al = _inputs(N, mirrored, False, 77)
    hot = np.random.default_rng(78).choice(N, 40, replace=False)
    al[hot] = -np.geomspace(1.0, 60.0, hot.size)
    kw = dict(n_steps=n, z_max=h * n, gamma=gam, alpha=al, a0=a0, check_nan=True, exact_step=True, extra_flags=LANES[lname])
    every = nat.sweep_host(db, save_every=1, want_traj=True, **kw)
    bad = every["first_bad_step"]
    assert (bad >= 0).sum() >= 20 and len(set(bad[bad >= 0])) >= 8 and (np.delete(bad, hot) == -1).all()
    ok = bad < 0
    for se in (7, 64, 1000):
        got = nat.sweep_host(db, save_every=se, **kw)
        assert np.array_equal(got["first_bad_step"], bad), se
        last = n // se * se
        assert same_bits(got["a_end"][ok], every["traj"][ok, last, :]), se


def test_drift_over_the_headline_run(oracle):
    """64 points of the headline sweep (every 1024th of its 65 536 dbeta values, its amplitudes and constants), 1e5 steps: the
    modulus of the rounded rotator accumulates in the sidebands for the whole run (<= 5.5e-17 per step) with no re-seed to
    reset it.  Bar: the project's 1e-9; the measured figure is in the module docstring."""
    db = np.linspace(-0.05, 0.05, 65_536)[::1024]
    a0 = np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(complex)
    kw = dict(z_max=1000.0, save_every=10, gamma=GAMMA, alpha=1.15e-4, a0=a0)
    ref = oracle.sweep(db, n=100_000, **kw)
    got = nat.sweep_host(db, n_steps=100_000, extra_flags=nat.OPT_ONE_LANE, **kw)
    err_a, err_p = rel_err(got["a_end"], ref["a_end"]), rel_err(got["p_max"], ref["p_max"])
    print(f"drift, 64 points x 1e5 steps: a_end rel err {err_a:.3e}, p_max rel err {err_p:.3e}")
    assert (got["first_bad_step"] == -1).all()
    assert err_a < RTOL_F64 and err_p < RTOL_F64
