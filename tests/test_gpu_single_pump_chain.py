"""Single-pump fibre chains on the GPU: what only this family has (psa_rk4_single_pump_chain_f64, sweep.rk4_chain_single_pump,
simulation.run_concatenated_single_pump_simulation, scan_mismtach.scan_single_pump_copier_psa_phase) against the NumPy
restatement tests/single_pump_chain_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest wave).  What every
wave-summary chain owes its caller is in tests/test_gpu_wave_chain.py.

* one span is psa_rk4_single_pump_f64 bit for bit;
* a failure in span 2 is reported at the chain's step index, and its NaN stays in the summaries and the gain;
* the single-run form split against the unsplit run;
* the phase-scan driver against the copier - PSA closed form and against a direct chain call."""
import numpy as np
import pytest

import psa_amd._native as nat
import single_pump_chain_np as chain_np
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach, simulation
from psa_amd.sweep import FibreSpan, rk4_chain_single_pump
from wave_family import KEYS, fibre, power_err, rows, single_pump_inputs, wave_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("want_traj", [True, False], ids=["traj", "summary"])
def test_one_span_is_the_sweep_bit_for_bit(want_traj):
    n = 37
    dbeta, a0, gamma, _ = single_pump_inputs(n, 1)
    kw = dict(save_every=10, a0=a0, want_traj=want_traj)
    ref = nat.single_pump_host(dbeta, n_steps=1000, z_max=100.0, gamma=gamma, alpha=1.15e-4, **kw)
    got = nat.single_pump_chain_host(dbeta[None], n_steps=[1000], seg_len=[100.0], gamma=gamma[None], alpha=[1.15e-4], **kw)
    for key in KEYS + ("traj",):
        if ref[key] is None:
            assert got[key] is None
        else:
            assert np.array_equal(got[key], ref[key], equal_nan=True), key
    assert got["first_bad_step"].shape == (n,) and (got["traj"] is not None) == want_traj


def test_first_bad_step_of_a_failure_in_span_two_is_cumulative():
    """Span 2 is past the RK4 stability edge at points 1 and 3 (gamma 300): the restatement fails there at local step 1, so
    the chain reports 400 + 1, exactly; the first failure wins when a third span follows behind a non-identity transfer."""
    n_pts = 5
    rng = np.random.default_rng(2)
    db = np.linspace(-0.02, 0.02, n_pts)
    gam2 = np.full(n_pts, 0.0115)
    gam2[[1, 3]] = 300.0
    a0 = np.sqrt(np.array([0.5, 1e-5, 1e-6])) * np.exp(1j * rng.uniform(-3, 3, (n_pts, 3)))
    spans = [(40.0, 400, db, 0.0115, 1e-4), (60.0, 600, db, gam2, 0.0)]
    ref = chain_np.chain(a0, spans, [np.ones(3)], 10)
    assert np.array_equal(ref["first_bad_step"], [-1, 401, -1, 401, -1])
    got = rk4_chain_single_pump(fibre(spans), a0=a0, transfers=[np.ones(3)], save_every=10, exact_step=True)
    third = spans + [(10.0, 100, db, 0.0115, 0.0)]
    tr3 = [np.ones(3), simulation.single_pump_mid_stage((-1.0, -3.0, 0.5), (0.4, 1.0, -2.0))]
    got3 = rk4_chain_single_pump(fibre(third), a0=a0, save_every=10, exact_step=True, transfers=tr3)
    for r in (got, got3):
        np.testing.assert_array_equal(r.first_bad_step, [-1, 401, -1, 401, -1])
        assert np.all(np.isnan(r.p_wave_max[[1, 3]])) and np.all(np.isfinite(r.p_wave_max[[0, 2, 4]]))
        g = r.signal_gain(1e-5, mode="max")
        assert np.all(np.isnan(g[[1, 3]])) and np.all(np.isfinite(g[[0, 2, 4]]))
    ok = [0, 2, 4]
    assert power_err(got.p_wave_max[ok], ref["p_wave_max"][ok]) < RTOL_F64 and wave_err(got.a_end[ok], ref["a_end"][ok]) < RTOL_F64
    # two (3,) transfers reach the C entry point as broadcast ones (PSA_BCAST_TRANSFER): gain and phase on every wave
    ref3 = chain_np.chain(a0, third, tr3, 10)
    assert np.array_equal(ref3["first_bad_step"], [-1, 401, -1, 401, -1])
    errs = (wave_err(got3.a_end[ok], ref3["a_end"][ok]), power_err(got3.p_wave_end[ok], ref3["p_wave_end"][ok]),
            power_err(got3.p_wave_max[ok], ref3["p_wave_max"][ok]))
    print(f"broadcast transfers, the finite points: a_end {errs[0]:.2e} p_wave_end {errs[1]:.2e} p_wave_max {errs[2]:.2e}")
    assert max(errs) < RTOL_F64


def test_single_run_form_split_against_the_unsplit_run(golden):
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    wp, ws = 2.0 * np.pi * 299792458.0 / 1550e-9, 2.0 * np.pi * 299792458.0 / 1537e-9
    kw = dict(omega_pump=wp, omega_signal=ws, p_in=[0.5, 1e-6, 1e-8], phase_in=[0.3, -1.0, 2.0], length_unit="km")
    fibre = dict(gamma=11.5, alpha=0.1, dispersion=d.scaled(1e-3))
    z1, A1 = simulation.run_single_pump_simulation(config.custom_simulation_config(z_max=0.5, dz=1e-3), **fibre, **kw)
    z2, A2 = simulation.run_concatenated_single_pump_simulation(
        [dict(fibre, cfg=config.custom_simulation_config(z_max=0.2, dz=1e-3)),
         dict(fibre, cfg=config.custom_simulation_config(z_max=0.3, dz=1e-3))], **kw)
    idx = rows([200, 300], 10)
    np.testing.assert_allclose(z2, z1[idx], rtol=1e-12, atol=1e-12)
    err = float(np.max(np.abs(A2 - A1[idx]) / np.max(np.abs(A1), axis=0)))
    print(f"split 200 + 300 steps against the unsplit run: {err:.2e}")
    assert A2.shape == (52, 3) and err < RTOL_F64
    # a provided dbeta takes the place of the dispersion
    from psa_amd.phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
    db = float(dispersion.delta_beta_from_omegas_array(np.array([wp, wp, ws, 2 * wp - ws]), d.scaled(1e-3), max_order=4))
    pm = dict(gamma=11.5, alpha=0.1, phase_matching_cfg=PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED,
                                                                            provided_delta_beta=db))
    z3, A3 = simulation.run_concatenated_single_pump_simulation(
        [dict(pm, cfg=config.custom_simulation_config(z_max=0.2, dz=1e-3)),
         dict(pm, cfg=config.custom_simulation_config(z_max=0.3, dz=1e-3))], **kw)
    assert np.array_equal(z3, z2) and float(np.max(np.abs(A3 - A2)) / np.max(np.abs(A2))) < 1e-12
    with pytest.raises(FloatingPointError, match=r"step 20\d \(span 1, local step \d\)"):
        simulation.run_concatenated_single_pump_simulation(
            [dict(fibre, cfg=config.custom_simulation_config(z_max=0.2, dz=1e-3)),
             dict(fibre, gamma=3e5, cfg=config.custom_simulation_config(z_max=0.3, dz=1e-3))], **kw)


def test_phase_scan_driver_against_the_closed_form_and_a_direct_call():
    """The lossless copier - PSA pair of the closed form (single_pump_chain_np.closed_form_case): the signal gain over 16
    pump phases is a + b cos(2 phi + const), so DFT bin 0 and 2 |bin 2| meet a and b at 1e-6 and every other bin is below
    1e-8 of bin 0.  A grid need not contain the extrema: the extinction is compared through the harmonics, where errors of
    1e-6 on a and b allow 10 log10(e) 1e-6 ((a + b)/(a - b) + 1) dB; the driver's own extinction_db is the grid's max - min."""
    c = chain_np.closed_form_case()
    cfgs = dict(psa_cfg=config.custom_simulation_config(z_max=c["psa"][1], dz=c["psa"][1] / c["steps"][1], save_every=50),
                copier_cfg=config.custom_simulation_config(z_max=c["copier"][1], dz=c["copier"][1] / c["steps"][0], save_every=50))
    kw = dict(gamma=c["gamma"], alpha=0.0, p_in=[c["p_pump"], c["p_seed"], 0.0], copier_delta_beta=c["copier"][0],
              phase=c["phases"], gain_mode="end", **cfgs)
    out = scan_mismtach.scan_single_pump_copier_psa_phase(psa_delta_beta=c["psa"][0], gain_unit="linear", **kw)
    assert out["gain"].shape == (16,) and out["gain_idler"].shape == (16,) and out["result"].n_steps == 500
    e0, e2, rest = chain_np.check_harmonics(out["gain"], c["a"], c["b"])
    F = np.fft.rfft(out["gain"]) / 16
    a, b = F[0].real, 2.0 * abs(F[2])
    ext, want_ext = 10.0 * np.log10((a + b) / (a - b)), 10.0 * np.log10((c["a"] + c["b"]) / (c["a"] - c["b"]))
    print(f"driver against the closed form: bin 0 {e0:.2e} bin 2 {e2:.2e} other bins {rest:.2e}; extinction {ext:.6f} dB "
          f"(closed form {want_ext:.6f}), on the grid {out['extinction_db']:.6f}")
    assert e0 < 1e-6 and e2 < 1e-6 and rest < 1e-8
    assert abs(ext - want_ext) < 10.0 * np.log10(np.e) * 1e-6 * ((c["a"] + c["b"]) / (c["a"] - c["b"]) + 1.0)
    assert out["extinction_db"] == pytest.approx(10.0 * np.log10(out["gain"].max() / out["gain"].min()), abs=1e-12)
    # on the grid the gain IS its DFT sum, so it stays within delta = 2 sum |other bins| of a + b cos(...): the grid's
    # max - min cannot pass the extinction of a + delta over a - delta (it reaches it when the grid holds the extrema)
    delta = 2.0 * sum(abs(F[j]) for j in range(1, F.size) if j != 2)
    assert out["gain_max_db"] - out["gain_min_db"] == out["extinction_db"]
    assert out["extinction_db"] <= 10.0 * np.log10((a + b + delta) / (a - b - delta)) + 1e-12
    # the idler carries the signal's photons: P_i = P_s - P_s(0) in the lossless chain
    assert np.max(np.abs(out["gain_idler"] - (out["gain"] - 1.0)) / out["gain"]) < 1e-9

    # K = 16 phases x M = 3 PSA mismatches in one launch per span, against the chain call it stands for
    G, P = c["gamma"], c["p_pump"]
    dbp = np.array([-2.5, -2.0, -1.5]) * G * P
    grid = scan_mismtach.scan_single_pump_copier_psa_phase(psa_delta_beta=dbp, gain_unit="dB", **kw)
    T = np.ones((16, 3), complex)
    T[:, 0] = np.exp(1j * c["phases"])
    direct = rk4_chain_single_pump([FibreSpan(c["copier"][1], n_steps=c["steps"][0], dbeta=c["copier"][0], gamma=G),
                                    FibreSpan(c["psa"][1], n_steps=c["steps"][1], dbeta=np.tile(dbp, 16), gamma=G)],
                                   a0=c["a0"], transfers=[np.repeat(T, 3, axis=0)], save_every=50)
    assert grid["gain"].shape == (16, 3) and np.array_equal(grid["psa_delta_beta"], dbp)
    assert wave_err(grid["result"].a_end, direct.a_end) < 1e-12 and np.all(grid["result"].first_bad_step == -1)
    want = direct.signal_gain(c["p_seed"], mode="end", unit="dB").reshape(16, 3)
    assert np.max(np.abs(grid["gain"] - want)) < 1e-9
    assert np.max(np.abs(10.0 ** (grid["gain"][:, 1] / 10.0) / out["gain"] - 1.0)) < 1e-12
    assert grid["extinction_db"] == pytest.approx(np.max(grid["gain"]) - np.min(grid["gain"]), abs=1e-12)
