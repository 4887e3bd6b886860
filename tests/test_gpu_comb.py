"""The multi-line ("frequency comb") sweep on the GPU (psa_rk4_comb_f64: M equally spaced lines with every FWM product among
them, one sweep point per lane) against the NumPy restatement tests/comb_np.py at the project's bar RTOL_F64 (1e-9 of the
point's largest line): parity and conservation, the tie to the single-pump kernel at M = 3, the loop's edges, the save stride,
both block sizes, dark lines, the failure index, the device entry and the drivers.  Shapes are the smallest that can go
wrong: 203 points are three full waves and a partial one, 1 500 steps are no multiple of RESYNC = 64, 32 805 points are the
first size that takes 256-thread workgroups; M = 3 and 12 are the ends of the range, 4 the smallest even comb, 7 the first
that needs more than 256 registers, 12 the one whose rotators live in LDS."""
import functools

import numpy as np
import pytest

import comb_np
import psa_amd._native as nat
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach, simulation, sweep
from psa_amd.frequency_plan import omega_from_lambda
from wave_family import COMB, KEYS, device_sweep, power_err, wave_err

pytestmark = pytest.mark.gpu

Z_MAX, N_STEPS = 300.0, 1500


@functools.lru_cache(maxsize=None)
def _parity_case(M, per_point, lossy):
    """Inputs and the restatement's every-step rows, computed once per case; any save stride is read off the rows."""
    kappa, a0, gamma, alpha = comb_np.random_inputs(203, M, 100 * M + 2 * per_point + lossy, per_point, lossy)
    ref = comb_np.integrate(a0, kappa, z_max=Z_MAX, n=N_STEPS, save_every=1, gamma=gamma, alpha=alpha, want_traj=True)
    assert (ref["first_bad_step"] == -1).all()
    return dict(kappa=kappa, a0=a0, gamma=gamma, alpha=alpha, rows=ref["traj"])


@pytest.mark.parametrize("save_every", [1, 7, 10])
@pytest.mark.parametrize("lossy", [True, False], ids=["lossy", "lossless"])
@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
@pytest.mark.parametrize("M", [3, 4, 7, 12])
def test_parity_and_conservation(M, per_point, lossy, save_every):
    c = _parity_case(M, per_point, lossy)
    r = nat.comb_host(c["kappa"], n_steps=N_STEPS, z_max=Z_MAX, save_every=save_every, gamma=c["gamma"], alpha=c["alpha"],
                      a0=c["a0"])
    saved = c["rows"][:, ::save_every]
    err_a = wave_err(r["a_end"], saved[:, -1])
    err_e = power_err(r["p_wave_end"], np.abs(saved[:, -1]) ** 2)
    err_m = power_err(r["p_wave_max"], np.max(np.abs(saved) ** 2, axis=1))
    print(f"M={M} per_point={per_point} lossy={lossy} save_every={save_every}: a_end {err_a:.2e} p_wave_end {err_e:.2e} "
          f"p_wave_max {err_m:.2e}")
    assert (r["first_bad_step"] == -1).all()
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64
    if not lossy:
        # the invariants of the truncated system, on the device's own output: sum P_m and sum m P_m, within 1e-9 of the total
        # (the restatement's own defect on these inputs is below 1e-11: the bar tests the kernel, not the step size)
        p_in = np.broadcast_to(np.abs(np.atleast_2d(c["a0"])) ** 2, (203, M))
        m = np.arange(M)
        total = p_in.sum(axis=1)
        d_p = np.max(np.abs(r["p_wave_end"].sum(axis=1) - total) / total)
        d_m = np.max(np.abs((m * r["p_wave_end"]).sum(axis=1) - (m * p_in).sum(axis=1)) / total)
        print(f"   conservation: sum P {d_p:.2e} sum m P {d_m:.2e}")
        assert d_p < 1e-9 and d_m < 1e-9


def test_three_lines_equal_the_single_pump_kernel():
    """Lines [1, 0, 2] are waves [p, s, i]; any kappa with kappa_0 + kappa_2 - 2 kappa_1 = dbeta: a random split."""
    N = 203
    rng = np.random.default_rng(8)
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, 3, 8)
    a0 = a0.copy()
    a0[:, 0] *= 10 ** rng.uniform(0, 3, N)                  # seeds up to 1 W: depleted points among them
    dbeta = kappa[:, 0] + kappa[:, 2] - 2.0 * kappa[:, 1]
    k1, k0 = rng.uniform(-0.01, 0.01, N), rng.uniform(-0.01, 0.01, N)
    split = np.column_stack([k0, k1, dbeta + 2.0 * k1 - k0])
    kw = dict(n_steps=N_STEPS, z_max=Z_MAX, save_every=7, gamma=gamma, alpha=alpha)
    ref = nat.single_pump_host(split[:, 0] + split[:, 2] - 2.0 * split[:, 1], a0=a0[:, [1, 0, 2]], **kw)
    got = nat.comb_host(split, a0=a0, **kw)
    err_a = wave_err(got["a_end"][:, [1, 0, 2]], ref["a_end"])
    err_m = power_err(got["p_wave_max"][:, [1, 0, 2]], ref["p_wave_max"])
    print(f"M = 3 against the single-pump kernel: a_end {err_a:.2e} p_wave_max {err_m:.2e}")
    assert err_a < RTOL_F64 and err_m < RTOL_F64
    assert (got["first_bad_step"] == -1).all() and (ref["first_bad_step"] == -1).all()


@pytest.mark.parametrize("save_every", [1, 4, 10])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 63, 64, 65, 130])
def test_loop_edges(n_steps, save_every):
    """One step, an odd count, the re-seed at 64 and one past it, n_steps < save_every (the only row is z = 0: the outputs are
    a0) and tails that only the check runs."""
    N, M = 70, 4
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, M, 77)
    z_max = 0.5 * n_steps
    r = nat.comb_host(kappa, n_steps=n_steps, z_max=z_max, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    assert (r["first_bad_step"] == -1).all()
    if n_steps < save_every:
        assert np.array_equal(r["a_end"], a0) and np.array_equal(r["p_wave_end"], r["p_wave_max"])
        assert np.max(np.abs(r["p_wave_end"] / np.abs(a0) ** 2 - 1.0)) < 1e-15
        return
    ref = comb_np.integrate(a0, kappa, z_max=z_max, n=n_steps, save_every=save_every, gamma=gamma, alpha=alpha)
    err_a, err_e, err_m = (wave_err(r["a_end"], ref["a_end"]), power_err(r["p_wave_end"], ref["p_wave_end"]),
                           power_err(r["p_wave_max"], ref["p_wave_max"]))
    print(f"n_steps={n_steps} save_every={save_every}: {err_a:.2e} {err_e:.2e} {err_m:.2e}")
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64


@functools.lru_cache(maxsize=None)
def _every_step_run():
    """70 points (one full wave and a ragged one), M = 4, 200 steps: every row of the trajectory, computed once."""
    kappa, a0, gamma, alpha = comb_np.random_inputs(70, 4, 31)
    kw = dict(n_steps=200, z_max=100.0, gamma=gamma, alpha=alpha, a0=a0)
    every = nat.comb_host(kappa, save_every=1, want_traj=True, **kw)
    assert (every["first_bad_step"] == -1).all() and np.isfinite(every["traj"].view(float)).all()
    ref = comb_np.integrate(a0, kappa, z_max=100.0, n=200, save_every=1, gamma=gamma, alpha=alpha, want_traj=True)
    assert np.array_equal(every["traj"][:, 0], a0) and wave_err(every["traj"], ref["traj"]) < RTOL_F64
    return kappa, kw, every["traj"]


@pytest.mark.parametrize("se", [2, 7, 64, 65, 200, 1000])
def test_the_stride_only_selects_rows(se):
    """The re-seeds sit on the absolute step grid, so which rows are saved does not change the computed trajectory: the rows
    at any stride are the same rows of the every-step run, bit for bit -- strides below, at and above RESYNC = 64, the whole
    run as one block, and no saved row at all (a_end is a0).  The summaries do not depend on want_traj."""
    n = 200
    kappa, kw, every = _every_step_run()
    r = nat.comb_host(kappa, save_every=se, want_traj=True, **kw)
    assert np.array_equal(r["traj"], every[:, ::se][:, :n // se + 1])
    assert np.array_equal(r["a_end"], every[:, n // se * se])
    dense = nat.comb_host(kappa, save_every=se, **kw)
    for key in KEYS:
        assert np.array_equal(dense[key], r[key]), key


def test_both_block_sizes_agree_bit_for_bit():
    """32 805 points are 513 waves: more than half the SIMDs, so the launch takes 256-thread workgroups; PSA_OPT_BLOCK64 forces
    single-wave workgroups on the same points."""
    N = 32805
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, 3, 5)
    kw = dict(n_steps=130, z_max=65.0, save_every=10, gamma=gamma, alpha=alpha, a0=a0)
    big = nat.comb_host(kappa, **kw)
    small = nat.comb_host(kappa, extra_flags=nat.OPT_BLOCK64, **kw)
    for key in KEYS:
        assert np.array_equal(big[key], small[key]), key
    ref = comb_np.integrate(a0, kappa, z_max=65.0, n=130, save_every=10, gamma=gamma, alpha=alpha)
    err = wave_err(big["a_end"], ref["a_end"])
    print(f"32 805 points: a_end {err:.2e}")
    assert err < RTOL_F64 and (big["first_bad_step"] == -1).all()


def test_the_lds_instantiations_agree_in_both_block_sizes():
    """M = 12 keeps its rotators in LDS, one column per lane of the workgroup: 64- and 256-thread workgroups, a ragged last
    one, bit for bit."""
    N = 32805
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, 12, 6)
    kw = dict(n_steps=70, z_max=35.0, save_every=10, gamma=gamma, alpha=alpha, a0=a0)
    big = nat.comb_host(kappa, **kw)
    small = nat.comb_host(kappa, extra_flags=nat.OPT_BLOCK64, **kw)
    for key in KEYS:
        assert np.array_equal(big[key], small[key]), key
    sel = slice(None, None, 257)
    ref = comb_np.integrate(a0[sel], kappa[sel], z_max=35.0, n=70, save_every=10, gamma=gamma[sel], alpha=alpha[sel])
    assert wave_err(big["a_end"][sel], ref["a_end"]) < RTOL_F64 and (big["first_bad_step"] == -1).all()


def test_dark_odd_lines_stay_dark():
    """With the odd lines dark every product that lands on an odd line has a dark factor: they stay exactly 0 on the device,
    and the even lines are the four-line comb of twice the spacing."""
    N = 203
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, 7, 3)
    a0 = a0.copy()
    a0[:, 1::2] = 0.0
    a0[:, 2] *= 30.0                                       # a strong line among the bright ones
    kw = dict(n_steps=N_STEPS, z_max=Z_MAX, save_every=10, gamma=gamma, alpha=alpha)
    seven = nat.comb_host(kappa, a0=a0, want_traj=True, **kw)
    four = nat.comb_host(kappa[:, ::2], a0=a0[:, ::2], **kw)
    assert np.all(seven["traj"][:, :, 1::2] == 0) and np.all(seven["p_wave_max"][:, 1::2] == 0)
    err = wave_err(seven["a_end"][:, ::2], four["a_end"])
    print(f"even lines of 7 against the 4-line run: {err:.2e}")
    assert err < RTOL_F64 and np.max(np.abs(four["p_wave_end"] / np.abs(a0[:, ::2]) ** 2 - 1.0)) > 1e-3


def _failing_inputs(M):
    """Abrupt blow-ups as in test_gpu_single_pump: a gain of 3.2 .. 12 per metre overflows within 25 steps."""
    N = 9
    kappa, a0, _, _ = comb_np.random_inputs(N, M, 41, per_point=False)
    return kappa, dict(n_steps=2000, z_max=200.0, save_every=10, gamma=0.0115, alpha=-np.linspace(3.2, 12, N), a0=a0)


@pytest.mark.parametrize("M", [4, 12])
def test_failure_index_is_exact_and_unchecked_runs_give_nan(M):
    kappa, kw = _failing_inputs(M)
    # the restatement's index, and that it does not hang on the last bits: unchanged under a 1e-9 perturbation of alpha
    al3 = np.concatenate([kw["alpha"], kw["alpha"] * (1 + 1e-9), kw["alpha"] * (1 - 1e-9)])
    ref = comb_np.integrate(kw["a0"], np.tile(kappa, (3, 1)), z_max=6.0, n=60, save_every=10, gamma=0.0115, alpha=al3)   # same step
    want = ref["first_bad_step"][:9]
    assert (want >= 0).all() and want.max() < 30
    assert np.array_equal(ref["first_bad_step"][9:18], want) and np.array_equal(ref["first_bad_step"][18:], want)
    got = nat.comb_host(kappa, **kw)
    print("device", got["first_bad_step"], "restatement", want)
    assert np.array_equal(got["first_bad_step"], want)
    # PSA_OPT_EXACT_STEP changes nothing: with or without it the index is the per-step one
    plain = nat.comb_host(kappa, check_nan=False, extra_flags=nat.OPT_CHECK_NAN, **kw)
    assert np.array_equal(plain["first_bad_step"], want)
    off = nat.comb_host(kappa, check_nan=False, **kw)
    assert (off["first_bad_step"] == -1).all()
    assert np.isnan(off["a_end"]).all() and np.isnan(off["p_wave_end"]).all() and np.isnan(off["p_wave_max"]).all()


@pytest.mark.parametrize("M", [4, 12])
def test_a_failing_lane_leaves_its_wave_neighbours_untouched(M):
    """One failing point among 202 healthy ones, in the middle of a wave.  Their outputs equal the run without the failure
    bit for bit; n_steps = 1 005 leaves a tail that only the check runs."""
    N, k = 203, 100
    kappa, a0, gamma, _ = comb_np.random_inputs(N, M, 3)
    alpha = np.full(N, 1.15e-4)
    kw = dict(n_steps=1005, z_max=100.5, save_every=10, gamma=gamma, a0=a0)
    clean = nat.comb_host(kappa, alpha=alpha, **kw)
    alpha_bad = alpha.copy()
    alpha_bad[k] = -8.0
    bad = nat.comb_host(kappa, alpha=alpha_bad, **kw)
    ok = np.arange(N) != k
    assert (clean["first_bad_step"] == -1).all() and (bad["first_bad_step"][ok] == -1).all()
    ref = comb_np.integrate(a0[k], kappa[k:k + 1], z_max=100.5 * 60 / 1005, n=60, save_every=10, gamma=gamma[k], alpha=-8.0)
    want = int(ref["first_bad_step"][0])
    assert want >= 0 and bad["first_bad_step"][k] == want
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(bad[key][ok], clean[key][ok]), key
        assert np.isnan(bad[key][k].view(float)).all(), key


@pytest.mark.parametrize("M", [5, 12])
def test_device_entry_equals_the_host_entry_bit_for_bit(M):
    torch = pytest.importorskip("torch")
    N = 203
    kappa, a0, gamma, _ = comb_np.random_inputs(N, M, 9)
    kw = dict(n_steps=500, z_max=100.0, save_every=10)
    host = nat.comb_host(kappa, gamma=gamma, alpha=1.15e-4, a0=a0, want_traj=True, **kw)
    flags = nat.BCAST_ALPHA | nat.OPT_CHECK_NAN
    got = device_sweep(torch, COMB, kappa.shape[1], kappa, gamma, 1.15e-4, a0, flags=flags, traj_ld=N, **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(got[key], host[key]), key


def test_padded_trajectory_rows_equal_the_dense_ones():
    """131 072 points put the line regions of a row 2 MiB apart: psa_traj_ld pads them by 272 points.  The padded `_dev` form,
    the dense one and the host form (which pads internally) agree bit for bit, and the padding is never written."""
    torch = pytest.importorskip("torch")
    N = 131072
    ld = nat.traj_ld(N)
    assert ld == N + 272
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, 3, 13)
    kw = dict(n_steps=5, z_max=2.5, save_every=2)
    flags = nat.OPT_CHECK_NAN
    dense = device_sweep(torch, COMB, kappa.shape[1], kappa, gamma, alpha, a0, flags=flags, traj_ld=N, **kw)
    padded = device_sweep(torch, COMB, kappa.shape[1], kappa, gamma, alpha, a0, flags=flags | nat.OPT_TRAJ_LD, traj_ld=ld, **kw)
    host = nat.comb_host(kappa, gamma=gamma, alpha=alpha, a0=a0, want_traj=True, **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(dense[key], padded[key]) and np.array_equal(dense[key], host[key]), key
    assert dense["traj"].shape == (N, 3, 3) and np.all(padded["pad"] == -7.0)


def test_two_blocks_on_one_device_equal_one_launch():
    N, M = 203, 6
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, M, 31)
    kw = dict(z_max=50.0, n_steps=500, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    one = sweep.rk4_sweep_comb(kappa, **kw)
    two = sweep.rk4_sweep_comb(kappa, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (N, 51, M) and np.array_equal(one.p_wave_in, np.abs(a0) ** 2)
    assert np.array_equal(one.total_power(), one.p_wave_end.sum(axis=1))


def _dispersion(golden):
    dv = golden("G11")["disp_m"]
    return dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])


def test_gain_driver_is_a_direct_call_on_the_kappa_it_reports(golden):
    """Two pumps 400 GHz apart on an eight-line 200 GHz grid, seeds and dark lines around them: scan_comb_gain is one
    rk4_sweep_comb call on the kappa it reports; the cascaded pump products at 2 w_1 - w_2 and 2 w_2 - w_1 (lines 1 and 7,
    dark at the input) come up, and a dark line has NaN gain."""
    d = _dispersion(golden)
    cfg = config.custom_simulation_config(z_max=300.0, dz=0.2)
    p = np.zeros((5, 8))
    p[:, 3] = p[:, 5] = 0.3
    p[:, 4] = 10.0 ** np.arange(-9, -4)
    dw = 2.0 * np.pi * 200e9
    out = scan_mismtach.scan_comb_gain(cfg=cfg, lambda_center_m=1550e-9, line_spacing=dw, p_lines=p, gamma=0.0115, alpha=1e-4,
                                       dispersion=d, gain_mode="end")
    omega, kappa, _ = simulation.comb_lines(omega_from_lambda(1550e-9), dw, 8, d)
    assert np.array_equal(out["kappa"], kappa) and np.array_equal(out["omega"], omega) and out["gain"].shape == (5, 8)
    direct = sweep.rk4_sweep_comb(np.tile(out["kappa"], (5, 1)), z_max=300.0, n_steps=1500, save_every=cfg.save_every, gamma=0.0115,
                                  alpha=1e-4, a0=np.sqrt(p).astype(complex))
    assert np.array_equal(out["result"].a_end, direct.a_end) and (out["first_bad_step"] == -1).all()
    assert np.array_equal(out["p_end"], direct.p_wave_end) and np.array_equal(out["p_max"], direct.p_wave_max)
    assert np.array_equal(out["gain"], direct.line_gain(p, mode="end"), equal_nan=True)
    bright = p > 0
    assert np.isnan(out["gain"][~bright]).all() and np.isfinite(out["gain"][bright]).all()
    assert np.all(out["p_end"][:, [1, 7]] > 1e-9)           # the cascaded pump products
    km = scan_mismtach.scan_comb_gain(cfg=config.custom_simulation_config(z_max=0.3, dz=2e-4), lambda_center_m=1550e-9,
                                      line_spacing=dw, p_lines=p, gamma=11.5, alpha=0.1, dispersion=d.scaled(1e-3),
                                      length_unit="km", gain_mode="end")
    assert np.allclose(km["kappa"], 1e3 * kappa, rtol=1e-12) and wave_err(km["result"].a_end, direct.a_end) < RTOL_F64


def test_single_run_driver_reproduces_a_direct_call(golden):
    d = _dispersion(golden)
    wc, dw = 2.0 * np.pi * 299792458.0 / 1550e-9, 2.0 * np.pi * 150e9
    p_in, ph = [1e-6, 0.3, 1e-4, 0.25, 0.0], [0.3, -1.0, 2.0, 0.5, 0.0]
    z, A = simulation.run_comb_simulation(config.custom_simulation_config(z_max=300.0, dz=0.1, save_every=7), gamma=0.0115,
                                          alpha=1e-4, omega_center=wc, line_spacing=dw, p_in=p_in, phase_in=ph, dispersion=d)
    _, kappa, _ = simulation.comb_lines(wc, dw, 5, d)
    direct = sweep.rk4_sweep_comb(kappa[None], z_max=300.0, n_steps=3000, save_every=7, gamma=0.0115, alpha=1e-4,
                                  a0=sweep.initial_amplitudes(p_in, ph), want_traj=True)
    assert A.shape == (429, 5) and np.array_equal(A, direct.traj[0]) and np.array_equal(z, np.linspace(0.0, 300.0, 3001)[::7])
    z_km, A_km = simulation.run_comb_simulation(config.custom_simulation_config(z_max=0.3, dz=1e-4, save_every=7), gamma=11.5,
                                                alpha=0.1, omega_center=wc, line_spacing=dw, p_in=p_in, phase_in=ph,
                                                dispersion=d.scaled(1e-3), length_unit="km")
    assert abs(z_km[-1] - 0.3 * 2996 / 3000) < 1e-15 and wave_err(A_km[None], direct.traj) < 1e-12   # a rounding apart
    with pytest.raises(FloatingPointError):
        # gamma P h = 3e4: the explicit step is unstable and overflows within a few steps
        simulation.run_comb_simulation(config.custom_simulation_config(z_max=300.0, dz=0.1), gamma=1e6, alpha=1e-4,
                                       omega_center=wc, line_spacing=dw, p_in=p_in, dispersion=d)
