"""Multi-channel fibre chains and saved rows on the GPU: what only this family has (psa_rk4_pairs_chain_f64,
sweep.rk4_chain_pairs, rk4_sweep_pairs(want_traj=True), scan_mismtach.scan_wdm_copier_psa_phase) against the NumPy restatement
tests/pairs_chain_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest wave).  What every wave-summary chain owes
its caller is in tests/test_gpu_wave_chain.py.

* the rows of one span for K = 1, 3, 16 (L = 2, 4, 16 lanes per point; 70 points with K = 3 are 280 lanes: more than one
  256-thread block, no multiple of 64), every step and every 7th of 130 saved; the summaries with and without rows bit-equal;
* one span without rows is psa_rk4_sweep_pairs_f64 bit for bit;
* K = 1 against rk4_chain on 4 waves and K = 2 against rk4_chain on 6 waves at 1e-10;
* permuting the pairs permutes the outputs;
* a failure in span 2 is reported at the chain's step index, exact and per save block, its neighbours untouched;
* devices=[0, 0] equals one device, for a chain and for a sweep's rows; the phase-scan driver against the dual-pump closed form and a
  direct chain call."""
import functools

import numpy as np
import pytest

import pairs_chain_np as chain_np
import psa_amd._native as nat
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach
from psa_amd.sweep import FibreSpan, rk4_chain, rk4_chain_pairs, rk4_sweep_pairs
from wave_family import KEYS, fibre, pairs_inputs, power_err, wave_err

pytestmark = pytest.mark.gpu


# ---- rows of one span -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_span(K):
    """70 points, 130 steps, every step saved by the restatement; any stride is read off its rows."""
    db, a0, gamma, alpha = pairs_inputs(70, K, 100 + K, (0.8, 1.6), (0.5, 2.0))
    ref = chain_np.integrate(a0, db, z_max=260.0, n=130, save_every=1, gamma=gamma, alpha=alpha)
    assert (ref["first_bad_step"] == -1).all()
    return a0, db, gamma, alpha, ref["traj"]


@pytest.mark.parametrize("save_every", [1, 7])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_rows_of_one_span_against_the_restatement(K, save_every):
    a0, db, gamma, alpha, rows = _one_span(K)
    want = rows[:, ::save_every]
    kw = dict(z_max=260.0, n_steps=130, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    got = rk4_sweep_pairs(db, want_traj=True, **kw)
    assert got.traj.shape == want.shape == (70, 130 // save_every + 1, 2 + 2 * K)
    errs = (wave_err(got.traj, want), wave_err(got.a_end, want[:, -1]), power_err(got.p_wave_end, np.abs(want[:, -1]) ** 2),
            power_err(got.p_wave_max, np.max(np.abs(want) ** 2, axis=1)))
    print(f"K = {K}, save_every = {save_every}: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} "
          f"p_wave_max {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    assert np.array_equal(got.traj[:, 0], a0) and np.array_equal(got.traj[:, -1], got.a_end)
    lean = rk4_sweep_pairs(db, **kw)
    assert lean.traj is None
    for key in KEYS:
        assert np.array_equal(getattr(lean, key), getattr(got, key)), key


@pytest.mark.parametrize("K", [1, 3, 16])
def test_one_span_without_rows_is_the_sweep_bit_for_bit(K):
    a0, db, gamma, alpha, _ = _one_span(K)
    kw = dict(save_every=10, a0=a0)
    ref = nat.sweep_pairs_host(db, n_steps=130, z_max=260.0, gamma=gamma, alpha=1.15e-4, **kw)
    got = nat.pairs_chain_host(db[None], n_steps=[130], seg_len=[260.0], gamma=gamma[None], alpha=[1.15e-4], **kw)
    for key in KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    assert got["traj"] is None and got["first_bad_step"].shape == (70,)


# ---- K = 1 and K = 2 are the 4- and the 6-wave chain ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2])
def test_one_and_two_pairs_against_rk4_chain(K):
    """Three lossy spans with per-point transfers (the broadcast one tiled); the kernels order the triple products differently,
    so they agree to rounding: 1e-10 of the point's largest wave on inputs that tests/test_pairs_chain_host.py shows to be
    well conditioned (a 1e-14 perturbation moves the rows by less than 1e-12)."""
    a0, spans, transfers = chain_np.lossy_case(70, K, seed=21, steps=(60, 100, 40))
    transfers = [np.broadcast_to(t, a0.shape) for t in transfers]
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    got = rk4_chain_pairs(fibre(spans), **kw)
    other = [FibreSpan(L, n_steps=n, dbeta=db[:, 0], dbeta2=(db[:, 1] if K == 2 else None), gamma=g, alpha=al)
             for L, n, db, g, al in spans]
    ref = rk4_chain(other, **kw)
    waves = rk4_chain(other, **dict(kw, want_traj=False, wave_summary=True))   # the per-wave summary takes no trajectory
    errs = (wave_err(got.traj, ref.traj), wave_err(got.a_end, ref.a_end), power_err(got.p_wave_end, waves.p_wave_end),
            power_err(got.p_wave_max, waves.p_wave_max))
    print(f"K = {K} against rk4_chain on {2 + 2 * K} waves: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} "
          f"p_wave_max {errs[3]:.2e}")
    assert got.traj.shape == ref.traj.shape == (70, 4 + 6 + 3, 2 + 2 * K) and max(errs) < 1e-10
    assert np.array_equal(got.first_bad_step, ref.first_bad_step) and np.array_equal(got.z_out, ref.z_out)


def test_permuting_the_pairs_permutes_the_outputs():
    """K = 5 (three padding lanes), two spans: pair k moved to lane perm[k].  The sums over the pairs are formed in another
    order, so the outputs agree to rounding (RTOL_F64), not bit for bit."""
    N, K = 40, 5
    a0, spans, transfers = chain_np.lossy_case(N, K, seed=9, steps=(100, 60), lengths=(250.0, 150.0))
    transfers = transfers[:1]
    perm = np.array([3, 0, 4, 2, 1])
    wave = np.concatenate([[0, 1], np.stack([2 + 2 * perm, 3 + 2 * perm], axis=1).ravel()])
    kw = dict(save_every=20, want_traj=True)
    base = rk4_chain_pairs(fibre(spans), a0=a0, transfers=transfers, **kw)
    moved = rk4_chain_pairs(fibre([(L, n, db[:, perm], g, al) for L, n, db, g, al in spans]), a0=a0[:, wave],
                            transfers=[t[:, wave] for t in transfers], **kw)
    errs = (wave_err(moved.traj, base.traj[:, :, wave]), wave_err(moved.a_end, base.a_end[:, wave]),
            power_err(moved.p_wave_max, base.p_wave_max[:, wave]), power_err(moved.p_wave_end, base.p_wave_end[:, wave]))
    print(f"permuted pairs: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_max {errs[2]:.2e} p_wave_end {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    ref = chain_np.chain(a0, spans, transfers, 20)
    assert wave_err(base.traj, ref["rows"]) < RTOL_F64


def test_first_bad_step_of_a_failure_in_span_two_is_cumulative():
    """Span 2 is past the RK4 stability edge at points 1 and 3 (gamma 300): the restatement fails there at local step 1
    (tests/test_pairs_chain_host.py), so the chain reports 400 + 1 exactly and 400 + 9, the last step of the save block,
    without exact_step.  The five points share one 64-lane wave (4 lanes each): the healthy ones are untouched."""
    a0, spans = chain_np.failing_case()
    ref = chain_np.chain(a0, spans, [np.ones(8)], 10)
    assert np.array_equal(ref["first_bad_step"], [-1, 401, -1, 401, -1])
    kw = dict(a0=a0, transfers=[np.ones(8)], save_every=10)
    got = rk4_chain_pairs(fibre(spans), exact_step=True, **kw)
    block = rk4_chain_pairs(fibre(spans), exact_step=False, **kw)
    np.testing.assert_array_equal(got.first_bad_step, [-1, 401, -1, 401, -1])
    np.testing.assert_array_equal(block.first_bad_step, [-1, 409, -1, 409, -1])
    ok = [0, 2, 4]
    for r in (got, block):
        assert np.all(np.isnan(r.p_wave_max[[1, 3]])) and np.all(np.isfinite(r.p_wave_max[ok]))
        g = r.channel_gain(np.full(3, 1e-5), mode="max")
        assert np.all(np.isnan(g[[1, 3]])) and np.all(np.isfinite(g[ok]))
        errs = (wave_err(r.a_end[ok], ref["a_end"][ok]), power_err(r.p_wave_end[ok], ref["p_wave_end"][ok]),
                power_err(r.p_wave_max[ok], ref["p_wave_max"][ok]))
        assert max(errs) < RTOL_F64
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(getattr(got, key)[ok], getattr(block, key)[ok]), key


# ---- devices ----------------------------------------------------------------------------------------------------------------
def test_two_devices_equal_one():
    a0, spans, transfers = chain_np.lossy_case(41, 3, steps=(60, 100, 40))
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    one = rk4_chain_pairs(fibre(spans), **kw)
    two = rk4_chain_pairs(fibre(spans), devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (41, 4 + 6 + 3, 8)
    # the sweep's rows split the same way
    a0, db, gamma, alpha, _ = _one_span(3)
    kw = dict(z_max=260.0, n_steps=130, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    one, two = rk4_sweep_pairs(db, **kw), rk4_sweep_pairs(db, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key


# ---- the phase scan -------------------------------------------------------------------------------------------------------
def test_phase_scan_driver_against_the_closed_form_and_a_direct_call():
    """The lossless WDM copier - PSA link of pairs_chain_np.wdm_case: K = 4 channels, 1e-12 W seeds, dark idlers, alpha = 0,
    F = 16 pump phases.  Every channel's gain is a_k + b_k cos(2 phi + const) with the dual-pump closed form (g_k^2 = 4 gamma^2
    P1 P2 - (kappa_k/2)^2, kappa_k = dbeta_k + gamma (P1 + P2)): DFT bin 0 and 2 |bin 2| meet a_k and b_k at BAR_BIN = 7.1e-8
    and every other bin stays below BAR_REST = 5.9e-10 of bin 0 -- ten times what the NumPy restatement leaves at the same
    step counts (tests/test_pairs_chain_host.py).  The scan equals the chain call it stands for to 1e-12."""
    c = chain_np.wdm_case()
    disp = dispersion.DispersionParams(**c["disp"])
    (Lc, Lp), (nc, npsa) = c["lengths"], c["steps"]
    kw = dict(psa_cfg=config.custom_simulation_config(z_max=Lp, dz=Lp / npsa, save_every=50),
              copier_cfg=config.custom_simulation_config(z_max=Lc, dz=Lc / nc, save_every=50), lambda_p1_m=c["lambda_p1_m"],
              lambda_p2_m=c["lambda_p2_m"], Omega=c["Omega"], p_pump=[c["p_pump"]] * 2, p_signal=[c["p_seed"]] * 4, p_idler=0.0,
              gamma=c["gamma"], alpha=0.0, dispersion=disp, phase=c["phases"], phase_wave="pumps", gain_mode="end")
    out = scan_mismtach.scan_wdm_copier_psa_phase(gain_unit="linear", **kw)
    assert out["gain"].shape == out["idler"].shape == (16, 4) and out["dbeta"].shape == (2, 4) and out["result"].n_steps == 500
    assert np.array_equal(out["dbeta"][0], out["dbeta"][1]) and np.all(out["first_bad_step"] == -1)
    a, b = chain_np.closed_form_gain(out["dbeta"][0], Lc, out["dbeta"][1], Lp, c["gamma"], c["p_pump"], c["p_pump"])
    for k in range(4):
        e0, e2, rest = chain_np.check_harmonics(out["gain"][:, k], a[k], b[k])
        print(f"channel {k}: gain {a[k]:.3f} +- {b[k]:.3f}; bin 0 {e0:.2e} bin 2 {e2:.2e} other bins {rest:.2e}")
        assert e0 < c["BAR_BIN"] and e2 < c["BAR_BIN"] and rest < c["BAR_REST"]
    # the idlers carry their signals' photons: P_i = P_s - P_s(0) in the lossless chain
    assert np.max(np.abs(out["idler"] - (out["gain"] - 1.0)) / out["gain"]) < 1e-9
    in_db = scan_mismtach.scan_wdm_copier_psa_phase(gain_unit="dB", **kw)
    assert np.max(np.abs(10.0 ** (in_db["gain"] / 10.0) / out["gain"] - 1.0)) < 1e-12
    for key, want in (("gain_max_db", in_db["gain"].max(axis=0)), ("gain_min_db", in_db["gain"].min(axis=0)),
                      ("extinction_db", in_db["gain"].max(axis=0) - in_db["gain"].min(axis=0))):
        assert out[key].shape == (4,) and np.array_equal(in_db[key], want) and np.array_equal(out[key], want), key
    # the chain call the scan stands for
    T = np.ones((16, 10), complex)
    T[:, :2] = np.exp(1j * c["phases"])[:, None]
    a_in = np.sqrt(np.array([c["p_pump"]] * 2 + [c["p_seed"], 0.0] * 4)).astype(complex)
    direct = rk4_chain_pairs([FibreSpan(Lc, n_steps=nc, dbeta=np.tile(out["dbeta"][0], (16, 1)), gamma=c["gamma"]),
                              FibreSpan(Lp, n_steps=npsa, dbeta=np.tile(out["dbeta"][1], (16, 1)), gamma=c["gamma"])],
                             a0=a_in, transfers=[T], save_every=50)
    assert wave_err(out["result"].a_end, direct.a_end) < 1e-12
    assert np.max(np.abs(out["gain"] / direct.channel_gain(np.full(4, c["p_seed"]), mode="end", unit="linear") - 1.0)) < 1e-12
