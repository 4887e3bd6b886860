"""The single-pump three-wave sweep on the GPU (psa_rk4_single_pump_f64: one pump, a signal and an idler, one sweep point per
lane) against the NumPy restatement tests/single_pump_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest wave):
parity and conservation, the loop's edges, both block sizes, the closed-form ties, the failure index, trajectory rows and the
plumbing up to the drivers.  Shapes are the smallest that can go wrong: 203 points are three full waves and a partial one,
1 500 steps are no multiple of RESYNC = 64, 32 805 points are the first size that takes 256-thread workgroups."""
import functools

import numpy as np
import pytest

import psa_amd._native as nat
import single_pump_np
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach, simulation, sweep
from single_pump_np import GAMMA, LENGTH, P_PUMP
from wave_family import KEYS, SINGLE_PUMP, device_sweep, power_err, wave_err

pytestmark = pytest.mark.gpu

ALPHA = 1.15e-4


def _inputs(N, seed, per_point, lossy):
    """Random phases, seeds from 1e-12 to 1e-2 W (undepleted and strongly depleted points share a wave), dbeta across the
    gain band."""
    rng = np.random.default_rng(seed)
    dbeta = rng.uniform(-4.5, 0.5, N) * GAMMA * P_PUMP
    if per_point:
        p = np.column_stack([rng.uniform(0.3, 0.6, N), 10 ** rng.uniform(-12, -2, N), 10 ** rng.uniform(-12, -2, N)])
        a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))
        gamma = GAMMA * rng.uniform(0.9, 1.1, N)
        alpha = ALPHA * rng.uniform(0.5, 1.5, N) if lossy else np.zeros(N)
    else:
        a0 = np.sqrt(np.array([P_PUMP, 1e-4, 1e-7])) * np.exp(1j * rng.uniform(-3, 3, 3))
        gamma, alpha = GAMMA, (ALPHA if lossy else 0.0)
    return dbeta, a0, gamma, alpha


@functools.lru_cache(maxsize=None)
def _parity_case(per_point, lossy):
    """Inputs and the restatement's every-step rows, computed once per case; any save stride is read off the rows."""
    dbeta, a0, gamma, alpha = _inputs(203, 10 + 2 * per_point + lossy, per_point, lossy)
    ref = single_pump_np.integrate(a0, dbeta, z_max=LENGTH, n=1500, save_every=1, gamma=gamma, alpha=alpha, want_traj=True)
    assert (ref["first_bad_step"] == -1).all()
    return dict(dbeta=dbeta, a0=a0, gamma=gamma, alpha=alpha, rows=ref["traj"])


@pytest.mark.parametrize("save_every", [1, 7, 10])
@pytest.mark.parametrize("lossy", [True, False], ids=["lossy", "lossless"])
@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
def test_parity_and_conservation(per_point, lossy, save_every):
    c = _parity_case(per_point, lossy)
    r = nat.single_pump_host(c["dbeta"], n_steps=1500, z_max=LENGTH, save_every=save_every, gamma=c["gamma"], alpha=c["alpha"],
                             a0=c["a0"])
    saved = c["rows"][:, ::save_every]
    err_a = wave_err(r["a_end"], saved[:, -1])
    err_e = power_err(r["p_wave_end"], np.abs(saved[:, -1]) ** 2)
    err_m = power_err(r["p_wave_max"], np.max(np.abs(saved) ** 2, axis=1))
    print(f"per_point={per_point} lossy={lossy} save_every={save_every}: a_end {err_a:.2e} p_wave_end {err_e:.2e} "
          f"p_wave_max {err_m:.2e}")
    assert (r["first_bad_step"] == -1).all()
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64
    # the invariants, on the device's own output: the total (times e^{alpha z}), and without loss P_s - P_i and P_p + 2 P_s
    z_end = LENGTH * (1500 // save_every * save_every) / 1500
    p_in = np.broadcast_to(np.abs(np.atleast_2d(c["a0"])) ** 2, (203, 3))
    p = r["p_wave_end"] * np.exp(np.broadcast_to(c["alpha"], (203,)) * z_end)[:, None]
    total = p_in.sum(axis=1)
    d_total = np.max(np.abs(p.sum(axis=1) - total) / total)
    d_mr = np.max(np.abs((p[:, 1] - p[:, 2]) - (p_in[:, 1] - p_in[:, 2])) / total)
    d_ps = np.max(np.abs((p[:, 0] + 2 * p[:, 1]) - (p_in[:, 0] + 2 * p_in[:, 1])) / total)
    print(f"   conservation: total {d_total:.2e} P_s - P_i {d_mr:.2e} P_p + 2 P_s {d_ps:.2e}")
    assert d_total < 1e-9 and d_mr < 1e-9 and d_ps < 1e-9       # uniform loss scales all three alike


@pytest.mark.parametrize("save_every", [1, 4, 10])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 5, 63, 64, 65, 130])
def test_loop_edges(n_steps, save_every):
    """One step, an odd count, the re-seed at 64 and one past it, n_steps < save_every (the only row is z = 0: the outputs are
    a0) and tails that only the check runs."""
    N = 70
    dbeta, a0, gamma, alpha = _inputs(N, 77, True, True)
    z_max = 0.5 * n_steps
    r = nat.single_pump_host(dbeta, n_steps=n_steps, z_max=z_max, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    assert (r["first_bad_step"] == -1).all()
    if n_steps < save_every:
        assert np.array_equal(r["a_end"], a0) and np.array_equal(r["p_wave_end"], r["p_wave_max"])
        assert np.max(np.abs(r["p_wave_end"] / np.abs(a0) ** 2 - 1.0)) < 1e-15
        return
    ref = single_pump_np.integrate(a0, dbeta, z_max=z_max, n=n_steps, save_every=save_every, gamma=gamma, alpha=alpha)
    err_a, err_e, err_m = (wave_err(r["a_end"], ref["a_end"]), power_err(r["p_wave_end"], ref["p_wave_end"]),
                           power_err(r["p_wave_max"], ref["p_wave_max"]))
    print(f"n_steps={n_steps} save_every={save_every}: {err_a:.2e} {err_e:.2e} {err_m:.2e}")
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64


def test_both_block_sizes_agree_bit_for_bit():
    """32 805 points are 513 waves: more than half the SIMDs, so the launch takes 256-thread workgroups; PSA_OPT_BLOCK64 forces
    single-wave workgroups on the same points."""
    N = 32805
    dbeta, a0, gamma, alpha = _inputs(N, 5, True, True)
    kw = dict(n_steps=130, z_max=65.0, save_every=10, gamma=gamma, alpha=alpha, a0=a0)
    big = nat.single_pump_host(dbeta, **kw)
    small = nat.single_pump_host(dbeta, extra_flags=nat.OPT_BLOCK64, **kw)
    for key in KEYS:
        assert np.array_equal(big[key], small[key]), key
    ref = single_pump_np.integrate(a0, dbeta, z_max=65.0, n=130, save_every=10, gamma=gamma, alpha=alpha)
    err = wave_err(big["a_end"], ref["a_end"])
    print(f"32 805 points: a_end {err:.2e}")
    assert err < RTOL_F64 and (big["first_bad_step"] == -1).all()


def test_closed_form_gain_on_the_device():
    """The undepleted-pump closed form G = 1 + (gamma P / g)^2 sinh^2(g L): bar 1e-6 on G and on the idler's G - 1."""
    c = single_pump_np.analytic_case()
    r = nat.single_pump_host(c["dbeta"], n_steps=c["n"], z_max=c["z_max"], save_every=c["n"], gamma=GAMMA, alpha=0.0, a0=c["a0"])
    G, Gi = r["p_wave_end"][:, 1] / c["p_seed"], r["p_wave_end"][:, 2] / c["p_seed"]
    err_s, err_i = np.max(np.abs(G / c["gain"] - 1.0)), np.max(np.abs(Gi / (c["gain"] - 1.0) - 1.0))
    print(f"closed form on the device: signal {err_s:.2e} idler {err_i:.2e}")
    assert err_s < 1e-6 and err_i < 1e-6 and (r["first_bad_step"] == -1).all()


def test_dark_sidebands_leave_self_phase_modulation():
    """Sidebands exactly 0; the pump follows exp(-alpha z / 2) exp(i gamma P_0 L_eff) within 1e-9."""
    r = nat.single_pump_host([0.013], n_steps=10_000, z_max=LENGTH, save_every=10, gamma=GAMMA, alpha=ALPHA,
                             a0=np.array([np.sqrt(P_PUMP), 0, 0], complex))
    leff = (1.0 - np.exp(-ALPHA * LENGTH)) / ALPHA
    want = np.sqrt(P_PUMP) * np.exp(-0.5 * ALPHA * LENGTH) * np.exp(1j * GAMMA * P_PUMP * leff)
    err = abs(r["a_end"][0, 0] - want) / abs(want)
    print(f"SPM: {err:.2e}")
    assert err < 1e-9 and np.all(r["a_end"][0, 1:] == 0) and np.all(r["p_wave_max"][0, 1:] == 0)


def _failing_inputs():
    """Abrupt blow-ups as in test_gpu_pairs: a gain of 3.2 .. 12 per metre overflows within 25 steps."""
    N = 9
    a0 = np.sqrt(np.array([0.5, 1e-5, 1e-5])).astype(complex)
    return np.linspace(-0.05, 0.05, N), dict(n_steps=2000, z_max=200.0, save_every=10, gamma=GAMMA, alpha=-np.linspace(3.2, 12, N),
                                             a0=a0)


def test_failure_index_exact_block_and_unchecked():
    dbeta, kw = _failing_inputs()
    # the restatement's index, and that it does not hang on the last bits: unchanged under a 1e-9 perturbation of alpha
    al3 = np.concatenate([kw["alpha"], kw["alpha"] * (1 + 1e-9), kw["alpha"] * (1 - 1e-9)])
    ref = single_pump_np.integrate(kw["a0"], np.tile(dbeta, 3), z_max=6.0, n=60, save_every=10, gamma=GAMMA, alpha=al3)   # same step
    want = ref["first_bad_step"][:9]
    assert (want >= 0).all() and want.max() < 30
    assert np.array_equal(ref["first_bad_step"][9:18], want) and np.array_equal(ref["first_bad_step"][18:], want)
    exact = nat.single_pump_host(dbeta, exact_step=True, **kw)
    print("exact", exact["first_bad_step"], "restatement", want)
    assert np.array_equal(exact["first_bad_step"], want)
    block = nat.single_pump_host(dbeta, exact_step=False, **kw)
    print("block", block["first_bad_step"])
    assert np.array_equal(block["first_bad_step"], want // 10 * 10 + 9)
    off = nat.single_pump_host(dbeta, check_nan=False, **kw)
    assert (off["first_bad_step"] == -1).all()
    assert np.isnan(off["a_end"]).all() and np.isnan(off["p_wave_end"]).all() and np.isnan(off["p_wave_max"]).all()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "block"])
def test_a_failing_lane_leaves_its_wave_neighbours_untouched(exact):
    """One failing point among 202 healthy ones, in the middle of a wave: the replay it triggers runs in its neighbours'
    lanes too.  Their outputs equal the run without the failure bit for bit; n_steps = 1 005 leaves a tail."""
    N, k = 203, 100
    dbeta, a0, gamma, _ = _inputs(N, 3, True, True)
    alpha = np.full(N, ALPHA)
    kw = dict(n_steps=1005, z_max=100.5, save_every=10, gamma=gamma, a0=a0, exact_step=exact)
    clean = nat.single_pump_host(dbeta, alpha=alpha, **kw)
    alpha_bad = alpha.copy()
    alpha_bad[k] = -8.0
    bad = nat.single_pump_host(dbeta, alpha=alpha_bad, **kw)
    ok = np.arange(N) != k
    assert (clean["first_bad_step"] == -1).all() and (bad["first_bad_step"][ok] == -1).all()
    ref = single_pump_np.integrate(a0[k], dbeta[k:k + 1], z_max=100.5 * 60 / 1005, n=60, save_every=10, gamma=gamma[k], alpha=-8.0)
    want = int(ref["first_bad_step"][0])
    assert want >= 0 and bad["first_bad_step"][k] == (want if exact else want // 10 * 10 + 9)
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(bad[key][ok], clean[key][ok]), key


@pytest.mark.parametrize("save_every", [1, 7, 10])
def test_trajectory_rows(save_every):
    """Row 0 is a0, every row within the bar of the restatement's, the last row is a_end bit for bit, and p_wave_max is the
    NaN-propagating maximum of |row|^2 (the kernel forms fma(x, x, y*y), NumPy rounds x*x + y*y twice: 2 ulp).  Point 5 fails,
    so NaN rows are among them."""
    N, n = 203, 130
    dbeta, a0, gamma, alpha = _inputs(N, 21, True, True)
    alpha = alpha.copy()
    alpha[5] = -9.0
    r = nat.single_pump_host(dbeta, n_steps=n, z_max=13.0, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    ref = single_pump_np.integrate(a0, dbeta, z_max=13.0, n=n, save_every=save_every, gamma=gamma, alpha=alpha, want_traj=True)
    traj = r["traj"]
    assert traj.shape == (N, n // save_every + 1, 3) and np.array_equal(traj[:, 0], a0)
    ok = np.arange(N) != 5
    err = wave_err(traj[ok], ref["traj"][ok])
    print(f"save_every={save_every}: rows {err:.2e}")
    assert err < RTOL_F64
    assert np.array_equal(traj[:, -1].view(float), r["a_end"].view(float), equal_nan=True)
    assert r["first_bad_step"][5] == ref["first_bad_step"][5] >= 0 and (r["first_bad_step"][ok] == -1).all()
    with np.errstate(all="ignore"):
        p_rows = np.max(traj.real ** 2 + traj.imag ** 2, axis=1)             # np.max propagates NaN
    assert np.isnan(r["p_wave_max"][5]).all() and np.isnan(p_rows[5]).all()
    assert np.max(np.abs(r["p_wave_max"][ok] / p_rows[ok] - 1.0)) < 5e-16
    dense = nat.single_pump_host(dbeta, n_steps=n, z_max=13.0, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    for key in KEYS:                                                        # the trajectory does not change the summary
        assert np.array_equal(dense[key], r[key], equal_nan=True), key


@functools.lru_cache(maxsize=None)
def _every_step_run():
    """70 points (one full wave and a ragged one), 200 steps: every row of the trajectory, computed once."""
    dbeta, a0, gamma, alpha = _inputs(70, 31, True, True)
    kw = dict(n_steps=200, z_max=100.0, gamma=gamma, alpha=alpha, a0=a0)
    every = nat.single_pump_host(dbeta, save_every=1, want_traj=True, **kw)
    assert (every["first_bad_step"] == -1).all() and np.isfinite(every["traj"].view(float)).all()
    return dbeta, kw, every["traj"]


@pytest.mark.parametrize("se", [2, 3, 7, 10, 31, 64, 65, 100, 200, 1000])
def test_the_stride_only_selects_rows(se):
    """The re-seeds sit on the absolute step grid, so which rows are saved does not change the computed trajectory: the rows
    at any stride are the same rows of the every-step run, bit for bit -- strides below, at and above RESYNC = 64, with and
    without an unsaved tail, the whole run as one block, and no saved row at all (a_end is a0)."""
    n = 200
    dbeta, kw, every = _every_step_run()
    r = nat.single_pump_host(dbeta, save_every=se, want_traj=True, **kw)
    assert np.array_equal(r["traj"], every[:, ::se][:, :n // se + 1])
    assert np.array_equal(r["a_end"], every[:, n // se * se])
    dense = nat.single_pump_host(dbeta, save_every=se, **kw)
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(dense[key], r[key]), key


@functools.lru_cache(maxsize=None)
def _graded_failures():
    """The inputs of test_gpu_lanes' replay test for this model: 60 of 331 points get a graded gain and blow up at step
    indices spread over the run.  With them the block-mode run at save_every = 1: a block is a step there, so its index is
    the per-step index and no replay is involved."""
    n, N = 450, 331
    rng = np.random.default_rng(7)
    db = rng.uniform(-0.05, 0.05, N)
    al = np.full(N, ALPHA)
    hot = rng.choice(N, 60, replace=False)
    al[hot] = -np.geomspace(1.0, 60.0, hot.size)
    kw = dict(n_steps=n, z_max=45.0, gamma=GAMMA, alpha=al, a0=np.sqrt([0.5, 1e-5, 1e-5]).astype(complex))
    per_step = nat.single_pump_host(db, save_every=1, exact_step=False, **kw)["first_bad_step"]
    return db, kw, per_step


@pytest.mark.parametrize("se", [7, 64, 1024])
def test_exact_index_equals_the_per_step_index(se):
    """The replay of a failing block repeats the forward pass, so the index it finds is the one a test after every step finds
    -- inside saved blocks, across the 64-step re-seeds and (se = 1024) in a run without a saved row.  Block mode names the
    block of that index, and finite points are bit-identical in both modes."""
    n = 450
    db, kw, per_step = _graded_failures()
    failed = per_step >= 0
    print(f"failing points {failed.sum()}, distinct indices {len(set(per_step[failed]))}, largest {per_step.max()}")
    assert failed.sum() >= 40 and len(set(per_step[failed])) >= 20 and per_step.max() >= 100
    got = nat.single_pump_host(db, save_every=se, exact_step=True, **kw)
    blk = nat.single_pump_host(db, save_every=se, exact_step=False, **kw)
    assert np.array_equal(got["first_bad_step"], per_step)
    exact, last_saved = per_step[failed], n // se * se
    assert np.array_equal(blk["first_bad_step"][failed], np.where(exact // se * se + se <= last_saved, exact // se * se + se - 1, n - 1))
    assert (blk["first_bad_step"][~failed] == -1).all()
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(got[key][~failed], blk[key][~failed]), key


def test_device_entry_equals_the_host_entry_bit_for_bit():
    torch = pytest.importorskip("torch")
    N = 203
    dbeta, a0, gamma, _ = _inputs(N, 9, True, True)
    kw = dict(n_steps=1000, z_max=100.0, save_every=10)
    host = nat.single_pump_host(dbeta, gamma=gamma, alpha=ALPHA, a0=a0, want_traj=True, **kw)
    flags = nat.BCAST_ALPHA | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP
    got = device_sweep(torch, SINGLE_PUMP, None, dbeta, gamma, ALPHA, a0, flags=flags, traj_ld=N, **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(got[key], host[key]), key


def test_padded_trajectory_rows_equal_the_dense_ones():
    """131 072 points put the wave regions of a row 2 MiB apart: psa_traj_ld pads them by 272 points.  The padded `_dev` form,
    the dense one and the host form (which pads internally) agree bit for bit, and the padding is never written."""
    torch = pytest.importorskip("torch")
    N = 131072
    ld = nat.traj_ld(N)
    assert ld == N + 272
    dbeta, a0, gamma, alpha = _inputs(N, 13, True, True)
    kw = dict(n_steps=5, z_max=2.5, save_every=2)
    flags = nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP
    dense = device_sweep(torch, SINGLE_PUMP, None, dbeta, gamma, alpha, a0, flags=flags, traj_ld=N, **kw)
    padded = device_sweep(torch, SINGLE_PUMP, None, dbeta, gamma, alpha, a0, flags=flags | nat.OPT_TRAJ_LD, traj_ld=ld, **kw)
    host = nat.single_pump_host(dbeta, gamma=gamma, alpha=alpha, a0=a0, want_traj=True, **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(dense[key], padded[key]) and np.array_equal(dense[key], host[key]), key
    assert dense["traj"].shape == (N, 3, 3) and np.all(padded["pad"] == -7.0)


def test_two_blocks_on_one_device_equal_one_launch():
    N = 203
    dbeta, a0, gamma, alpha = _inputs(N, 31, True, True)
    kw = dict(z_max=50.0, n_steps=500, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    one = sweep.rk4_sweep_single_pump(dbeta, **kw)
    two = sweep.rk4_sweep_single_pump(dbeta, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (N, 51, 3) and np.array_equal(one.p_wave_in, np.abs(a0) ** 2)


def _dispersion(golden):
    dv = golden("G11")["disp_m"]
    return dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])


def test_single_run_driver_reproduces_a_direct_call(golden):
    d = _dispersion(golden)
    cfg = config.custom_simulation_config(z_max=0.3, dz=1e-4, save_every=7)          # km: 3 000 steps, 429 rows
    wp = 2.0 * np.pi * 299792458.0 / 1550e-9
    ws = 2.0 * np.pi * 299792458.0 / 1537e-9
    p_in, ph = [0.5, 1e-6, 1e-8], [0.3, -1.0, 2.0]
    z, A = simulation.run_single_pump_simulation(cfg, gamma=11.5, alpha=0.1, omega_pump=wp, omega_signal=ws, p_in=p_in,
                                                 phase_in=ph, dispersion=d.scaled(1e-3), length_unit="km")
    db = float(dispersion.delta_beta_from_omegas_array(np.array([wp, wp, ws, 2 * wp - ws]), d, max_order=4))
    direct = sweep.rk4_sweep_single_pump([db], z_max=300.0, n_steps=3000, save_every=7, gamma=0.0115, alpha=1e-4,
                                         a0=sweep.initial_amplitudes(p_in, ph), want_traj=True)
    assert A.shape == (429, 3) and z.shape == (429,) and z[0] == 0.0 and abs(z[-1] - 0.3 * 2996 / 3000) < 1e-15
    assert wave_err(A[None], direct.traj) < 1e-12        # the km path divides gamma, alpha and beta_n by 1e3: a rounding apart
    z_m, A_m = simulation.run_single_pump_simulation(config.custom_simulation_config(z_max=300.0, dz=0.1, save_every=7),
                                                     gamma=0.0115, alpha=1e-4, omega_pump=wp, omega_signal=ws, p_in=p_in,
                                                     phase_in=ph, dispersion=d)
    assert np.array_equal(A_m, direct.traj[0]) and np.array_equal(z_m, np.linspace(0.0, 300.0, 3001)[::7])
    with pytest.raises(FloatingPointError):
        # gamma P h = 5e4: the explicit step is unstable and overflows within a few steps
        simulation.run_single_pump_simulation(config.custom_simulation_config(z_max=300.0, dz=0.1), gamma=1e6, alpha=1e-4,
                                              omega_pump=wp, omega_signal=ws, p_in=p_in, dispersion=d)


def test_gain_spectrum_driver(golden):
    """scan_single_pump_gain is one direct rk4_sweep_single_pump call on the mismatches it reports; an invalid plan gives NaN
    for that point alone; the peak sits at dbeta = -2 gamma P_p (the sweep's spacing there is 0.05 gamma P_p)."""
    d = _dispersion(golden)
    cfg = config.custom_simulation_config(z_max=300.0, dz=0.1)
    lam = np.concatenate([np.linspace(1530e-9, 1549.5e-9, 128), [-1.0, 700e-9]])   # a negative wavelength; an idler below 0
    out = scan_mismtach.scan_single_pump_gain(cfg=cfg, lambda_pump_m=1550e-9, lambda_signal_m=lam, p_pump=0.5, p_signal=1e-9,
                                              gamma=GAMMA, alpha=0.0, dispersion=d, gain_mode="end")
    ok = np.arange(130) < 128
    for key in ("gain", "idler", "pump_depletion", "dbeta"):
        assert out[key].shape == (130,) and np.isnan(out[key][~ok]).all() and np.isfinite(out[key][ok]).all(), key
    direct = sweep.rk4_sweep_single_pump(out["dbeta"][ok], z_max=300.0, n_steps=3000, save_every=cfg.save_every, gamma=GAMMA,
                                         alpha=0.0, a0=np.sqrt(np.array([0.5, 1e-9, 0.0])).astype(complex))
    assert np.array_equal(out["result"].a_end[ok], direct.a_end) and (out["first_bad_step"] == -1).all()
    assert np.array_equal(out["gain"][ok], direct.signal_gain(1e-9, mode="end"))
    assert np.array_equal(out["idler"][ok], direct.idler_conversion(1e-9, mode="end"))
    assert np.array_equal(out["pump_depletion"][ok], direct.pump_depletion())
    peak = out["dbeta"][np.nanargmax(out["gain"])] / (GAMMA * 0.5)
    want_db = 10 * np.log10(single_pump_np.analytic_gain(out["dbeta"][ok], GAMMA, 0.5, 300.0))
    print(f"peak at dbeta = {peak:.3f} gamma P; gain against the closed form {np.max(np.abs(out['gain'][ok] - want_db)):.2e} dB")
    assert abs(peak + 2.0) < 0.1
    assert np.max(np.abs(out["gain"][ok] - want_db)) < 1e-6      # a decade over the depletion term 2 G p_s / P_p = 1.4e-7 dB
