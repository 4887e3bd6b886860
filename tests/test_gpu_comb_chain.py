"""Multi-line ("comb") fibre chains on the GPU: what only this family has (psa_rk4_comb_chain_f64, sweep.rk4_chain_comb,
simulation.run_concatenated_comb_simulation, scan_mismtach.scan_comb_copier_psa_phase) against the NumPy restatement
tests/comb_chain_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest line).  What every wave-summary chain owes
its caller is in tests/test_gpu_wave_chain.py.

* one span is psa_rk4_comb_f64 bit for bit, with and without rows, M = 3 and 12;
* M = 3 against rk4_chain_single_pump at 1e-10;
* a failure in span 2 is reported at the chain's step index, its neighbours untouched, a third span changes nothing;
* the span driver against the unsplit single run; the phase-scan driver at M = 3 against the single-pump closed form and a
  direct chain call."""
import numpy as np
import pytest

import comb_chain_np as chain_np
import psa_amd._native as nat
import single_pump_chain_np
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach, simulation
from psa_amd.frequency_plan import omega_from_lambda
from psa_amd.sweep import FibreSpan, rk4_chain_comb, rk4_chain_single_pump
from wave_family import KEYS, fibre, power_err, rows, wave_err

pytestmark = pytest.mark.gpu


# ---- one span is the sweep --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_traj", [False, True], ids=["summary", "rows"])
@pytest.mark.parametrize("M", [3, 12])
def test_one_span_is_the_sweep_bit_for_bit(M, want_traj):
    """37 points x 130 steps: psa_rk4_comb_chain_f64 with S = 1 against psa_rk4_comb_f64, every output the same bits."""
    rng = np.random.default_rng(100 + M)
    N = 37
    kp, a0 = chain_np.random_kappa(rng, N, M), chain_np.random_a0(rng, N, M)
    gamma = chain_np.GAMMA * rng.uniform(0.8, 1.6, N)
    kw = dict(save_every=10, a0=a0, want_traj=want_traj)
    ref = nat.comb_host(kp, n_steps=130, z_max=260.0, gamma=gamma, alpha=1.15e-4, **kw)
    got = nat.comb_chain_host(kp[None], n_steps=[130], seg_len=[260.0], gamma=gamma[None], alpha=[1.15e-4], **kw)
    for key in KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    assert np.all(np.isfinite(got["a_end"])) and np.all(got["first_bad_step"] == -1)
    if want_traj:
        assert got["traj"].shape == (N, 14, M) and np.array_equal(got["traj"], ref["traj"])
    else:
        assert got["traj"] is None


# ---- three lines are the single-pump chain --------------------------------------------------------------------------------
def test_three_lines_against_rk4_chain_single_pump():
    """The lossy three-span case of the single-pump chain (300 points, 120 + 200 + 80 steps) on lines [s, p, i], every span's
    dbeta split at random into kappa_0 + kappa_2 - 2 kappa_1: the two kernels order their products differently, so they agree
    to rounding, 1e-10 of the point's largest wave."""
    case = single_pump_chain_np.lossy_case(300, steps=(120, 200, 80))
    a0, spans, transfers = chain_np.from_single_pump(case, np.random.default_rng(6))
    kw = dict(save_every=20, want_traj=True)
    got = rk4_chain_comb(fibre(spans), a0=a0, transfers=transfers, **kw)
    ref = rk4_chain_single_pump(fibre(case[1]), a0=case[0], transfers=case[2], **kw)
    o = [1, 0, 2]
    errs = (wave_err(got.traj, ref.traj[..., o]), wave_err(got.a_end, ref.a_end[:, o]), power_err(got.p_wave_end, ref.p_wave_end[:, o]),
            power_err(got.p_wave_max, ref.p_wave_max[:, o]))
    print(f"M = 3 against rk4_chain_single_pump: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} "
          f"p_wave_max {errs[3]:.2e}")
    assert got.traj.shape == ref.traj.shape == (300, 7 + 11 + 5, 3) and max(errs) < 1e-10
    assert np.array_equal(got.first_bad_step, ref.first_bad_step) and np.array_equal(got.z_out, ref.z_out)


# ---- a failure -------------------------------------------------------------------------------------------------------------
def test_first_bad_step_of_a_failure_in_span_two_is_cumulative():
    """Span 2 is past the RK4 stability edge at points 1 and 3 (gamma 300): the restatement fails there at local step 1
    (tests/test_comb_chain_host.py), so the chain reports 400 + 1 (the multi-line kernel tests after every step).  The healthy
    points are untouched, and a third span behind the failure changes nothing about it."""
    a0, spans = chain_np.failing_case()
    ref = chain_np.chain(a0, spans, [np.ones(4)], 10)
    assert np.array_equal(ref["first_bad_step"], [-1, 401, -1, 401, -1])
    got = rk4_chain_comb(fibre(spans), a0=a0, transfers=[np.ones(4)], save_every=10)
    np.testing.assert_array_equal(got.first_bad_step, ref["first_bad_step"])
    ok = [0, 2, 4]
    assert np.all(np.isnan(got.p_wave_max[[1, 3]])) and np.all(np.isfinite(got.p_wave_max[ok]))
    g = got.line_gain(np.abs(a0) ** 2, mode="max")
    assert np.all(np.isnan(g[[1, 3]])) and np.all(np.isfinite(g[ok]))
    errs = (wave_err(got.a_end[ok], ref["a_end"][ok]), power_err(got.p_wave_end[ok], ref["p_wave_end"][ok]),
            power_err(got.p_wave_max[ok], ref["p_wave_max"][ok]))
    assert max(errs) < RTOL_F64
    third = (10.0, 100, spans[0][2], chain_np.GAMMA, 0.0)
    more = rk4_chain_comb(fibre(spans + [third]), a0=a0, transfers=[np.ones(4)] * 2, save_every=10)
    np.testing.assert_array_equal(more.first_bad_step, ref["first_bad_step"])
    ref3 = chain_np.chain(a0, spans + [third], [np.ones(4)] * 2, 10)
    assert wave_err(more.a_end[ok], ref3["a_end"][ok]) < RTOL_F64 and power_err(more.p_wave_max[ok], ref3["p_wave_max"][ok]) < RTOL_F64


# ---- the span driver -------------------------------------------------------------------------------------------------------
def test_span_driver_against_the_unsplit_single_run():
    """run_concatenated_comb_simulation on one fibre cut into a 300 m and a 400 m span against run_comb_simulation on the 700 m
    fibre: the rows they share within RTOL_F64 of the largest line, z_out too."""
    d = dispersion.DispersionParams(omega_ref=2.0 * np.pi * 299792458.0 / 1554e-9, beta2=-2.3e-28, beta3=4.1e-41, beta4=-3.2e-55)
    kw = dict(omega_center=2.0 * np.pi * 299792458.0 / 1550e-9, line_spacing=2.0 * np.pi * 300e9, p_in=[1e-6, 2e-5, 0.2, 0.3, 0.0, 1e-5],
              phase_in=[0.3, -1.0, 0.0, 2.0, 0.0, 1.0])
    fibre = dict(gamma=0.0115, alpha=4.6e-5, dispersion=d)
    cfgs = [config.custom_simulation_config(z_max=L, dz=0.5) for L in (700.0, 300.0, 400.0)]
    z, A = simulation.run_comb_simulation(cfgs[0], **fibre, **kw)
    zc, Ac = simulation.run_concatenated_comb_simulation([dict(cfg=c, **fibre) for c in cfgs[1:]], **kw)
    idx = rows([600, 800], 10)
    assert Ac.shape == (61 + 81, 6) and A.shape == (141, 6)
    err = wave_err(Ac[None], A[idx][None])
    print(f"span driver against the single run: {err:.2e}")
    assert err < RTOL_F64
    np.testing.assert_allclose(zc, z[idx], rtol=1e-12, atol=1e-9)


# ---- the phase scan -------------------------------------------------------------------------------------------------------
def test_phase_scan_driver_against_the_closed_form_and_a_direct_call():
    """The lossless copier - PSA link of comb_chain_np.closed_form_case on three lines [s, p, i]: a 0.5 W pump, a 1e-12 W seed,
    the idler dark, F = 16 pump phases (phase_lines = the pump).  The signal gain is a + b cos(2 phi + const) with the
    single-pump closed form: DFT bin 0 meets a at 3.02e-8, 2 |bin 2| meets b at 3.32e-8 and every other bin stays below 1.75e-10
    of bin 0 -- ten times what the NumPy restatement leaves at the same step counts (tests/test_comb_chain_host.py).  The scan
    equals the chain call it stands for to 1e-12."""
    c = chain_np.closed_form_case()
    disp = dispersion.DispersionParams(omega_ref=omega_from_lambda(c["lambda_center_m"]), beta2=c["beta2"])
    (Lc, Lp), (nc, npsa) = c["lengths"], c["steps"]
    kw = dict(psa_cfg=config.custom_simulation_config(z_max=Lp, dz=Lp / npsa, save_every=50),
              copier_cfg=config.custom_simulation_config(z_max=Lc, dz=Lc / nc, save_every=50), lambda_center_m=c["lambda_center_m"],
              line_spacing=c["line_spacing"], p_lines=[c["p_seed"], c["p_pump"], 0.0], gamma=c["gamma"], alpha=0.0, dispersion=disp,
              phase=c["phases"], phase_lines=[1], gain_mode="end")
    out = scan_mismtach.scan_comb_copier_psa_phase(gain_unit="linear", **kw)
    assert out["gain"].shape == out["p_out"].shape == (16, 3) and out["kappa"].shape == (2, 3) and out["result"].n_steps == 500
    assert np.array_equal(out["kappa"][0], out["kappa"][1]) and np.all(out["first_bad_step"] == -1)
    kp = out["kappa"][0]
    np.testing.assert_allclose(kp[0] + kp[2] - 2.0 * kp[1], -2.0 * c["gamma"] * c["p_pump"], rtol=1e-11)
    e0, e2, rest = single_pump_chain_np.check_harmonics(out["gain"][:, 0], c["a"], c["b"])
    print(f"gain {c['a']:.3f} +- {c['b']:.3f}; bin 0 {e0:.2e} bin 2 {e2:.2e} other bins {rest:.2e}")
    assert e0 < c["BARS"][0] and e2 < c["BARS"][1] and rest < c["BARS"][2]
    # a line dark at the input has no gain; its power is the signal's photons: P_i = P_s - P_s(0) in the lossless chain
    assert np.isnan(out["gain"][:, 2]).all() and np.all(np.isfinite(out["gain"][:, :2]))
    assert np.max(np.abs(out["p_out"][:, 2] / c["p_seed"] - (out["gain"][:, 0] - 1.0)) / out["gain"][:, 0]) < 1e-9
    in_db = scan_mismtach.scan_comb_copier_psa_phase(gain_unit="dB", **kw)
    assert np.max(np.abs(10.0 ** (in_db["gain"][:, :2] / 10.0) / out["gain"][:, :2] - 1.0)) < 1e-12
    for key, want in (("gain_max_db", in_db["gain"].max(axis=0)), ("gain_min_db", in_db["gain"].min(axis=0)),
                      ("extinction_db", in_db["gain"].max(axis=0) - in_db["gain"].min(axis=0))):
        assert out[key].shape == (3,) and np.isnan(out[key][2]), key
        assert np.array_equal(in_db[key][:2], want[:2]) and np.array_equal(out[key][:2], want[:2]), key
    # the chain call the scan stands for
    T = np.ones((16, 3), complex)
    T[:, 1] = np.exp(1j * c["phases"])
    direct = rk4_chain_comb([FibreSpan(Lc, n_steps=nc, dbeta=np.tile(out["kappa"][0], (16, 1)), gamma=c["gamma"]),
                             FibreSpan(Lp, n_steps=npsa, dbeta=np.tile(out["kappa"][1], (16, 1)), gamma=c["gamma"])],
                            a0=c["a0"], transfers=[T], save_every=50)
    assert wave_err(out["result"].a_end, direct.a_end) < 1e-12
    assert np.max(np.abs(out["gain"][:, 0] / direct.line_gain(np.abs(c["a0"]) ** 2, mode="end", unit="linear")[:, 0] - 1.0)) < 1e-12
