"""The folded stage of the float64 mirrored z-loop (yaman_stage_mirrored with FOLD): stages 1, 2 and 4
multiply the UN-doubled product x*y by a doubled phase factor 2E instead of forming q_i = fma(x, y, y*x) = 2*RN(x*y).  The
identity is exact (tests/test_fold_identity.py), so the mirrored loop must still return the bits of the general loop -- also
where x*y is subnormal, where everything overflows at once, and in the replay of a failing block, which carries 2E across a
re-seed of the phase recurrence.  Two waves in one launch, as in tests/test_gpu_mirrored_waves.py: 64 mirrored points next to
the same 64 with one asymmetric lane, which takes the general loop.  PSA_OPT_ONE_LANE throughout."""
import numpy as np
import pytest

import psa_amd._native as nat

pytestmark = pytest.mark.gpu

GAMMA, ALPHA = 0.0115, 1.15e-4
I_IDLER = 40                                         # the asymmetric lane of the general wave
KEEP = np.array([k for k in range(64) if k != I_IDLER])
KEYS = ("a_end", "p_end", "p_max", "first_bad_step", "traj")
RESYNC = 64                                          # steps between two exact re-seeds of the float64 phase recurrence


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype.kind in "fc" else x


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _two_waves(a0_64, gamma=GAMMA, alpha=ALPHA):
    """points 0..63 = a0_64 (mirrored loop); points 64..127 the same with lane I_IDLER asymmetric (general loop)"""
    rng = np.random.default_rng(5)
    db64 = rng.uniform(-0.05, 0.05, 64)
    a0 = np.concatenate([a0_64, a0_64])
    a0[64 + I_IDLER, 3] = 1.5 * a0[64 + I_IDLER, 2]
    two = lambda v: np.r_[v, v] if np.ndim(v) else v   # noqa: E731
    return nat.sweep_host(np.r_[db64, db64], n_steps=200, z_max=20.0, save_every=7, gamma=two(gamma), alpha=two(alpha), a0=a0,
                          want_traj=True, check_nan=True, exact_step=True, extra_flags=nat.OPT_ONE_LANE)


def _small_sidebands():
    rng = np.random.default_rng(11)
    pump = np.sqrt(rng.uniform(0.2, 0.8, 64)) * np.exp(1j * rng.uniform(-3.1, 3.1, 64))
    side = 10.0 ** rng.uniform(-162, -155, 64) * np.exp(1j * rng.uniform(-3.1, 3.1, 64))
    return np.column_stack([pump, pump, side, side])


def test_subnormal_products_give_the_same_bits():
    """sidebands of 1e-155 ... 1e-162: every x*y of A3*A3 is subnormal (1e-310 ... 1e-324) or zero"""
    got = _two_waves(_small_sidebands())
    assert (got["first_bad_step"] == -1).all() and np.isfinite(got["a_end"]).all()
    assert (np.abs(got["a_end"][:, 2]) > 0).all()
    for k in KEYS:
        assert same_bits(got[k][KEEP], got[k][64 + KEEP]), k


def test_a_step_that_overflows_at_once_fails_in_both_loops():
    """gamma = 1e150: the first step is non-finite whatever the sidebands; only the index is contractual there"""
    got = _two_waves(_small_sidebands(), gamma=1e150)
    assert (got["first_bad_step"] == 0).all()
    assert np.array_equal(got["first_bad_step"][0:64], got["first_bad_step"][64:128])


def test_the_replay_carries_the_doubled_factor_past_a_reseed():
    """Lanes 0..31 amplify (alpha = -1.15 ... -1.3 per unit length) until the cubic terms overflow, somewhere between step 50
    and step 160 depending on the lane; the other lanes stay healthy.  With save_every = 7 the exact index comes from a
    replay of up to seven steps from the last saved row; for a point whose failing block contains step 64, 128 or 192 that
    replay re-seeds the phase factor, re-forms its double and runs the folded step behind it.  At least one such point must
    exist in the GENERAL wave (the ladder was laid out with the CPU oracle, which finds twenty); then both loops must name
    the same step for every point, and agree in every bit wherever a point has not failed yet."""
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(complex), (64, 1))
    alpha = np.full(64, ALPHA)
    alpha[0:32] = -np.linspace(1.15, 1.3, 32)
    got = _two_waves(a0, alpha=alpha)
    fb = got["first_bad_step"]
    failed = fb[64:128] >= 0
    crossing = failed & ((fb[64:128] // 7 * 7) // RESYNC != fb[64:128] // RESYNC)
    print("first_bad_step, general wave:", fb[64:128], " replays past a re-seed:", int(crossing.sum()))
    assert crossing.any() and (fb[64 + 32:128] == -1).all()
    assert np.array_equal(fb[0:64], fb[64:128])
    healthy = KEEP[fb[KEEP] == -1]
    for k in KEYS:
        assert same_bits(got[k][healthy], got[k][64 + healthy]), k
    for p in KEEP[fb[KEEP] >= 0]:                                    # a failing point: the rows saved before its bad step
        rows = fb[p] // 7 + 1
        assert same_bits(got["traj"][p, :rows], got["traj"][64 + p, :rows]), p
