"""The adaptive (RK45) sweep on the GPU: G18 (scipy's RK45 on the reference's RHS) through the three call levels, a seeded
random sweep against the NumPy restatement (tests/rk45_np.py), accuracy against a converged RK4 sweep and against an 80-bit
plain RK4 that is none of the project's GPU code, lane independence,
the failure statuses, the device form (also replayed from a captured graph), the dense rows and the lossless path."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import psa_amd._native as nat
import rk45_np
from truth_cases import rk45_random_points as _random_points
from psa_amd.config import AdaptiveConfig, custom_simulation_config
from psa_amd.integrators import integrate_adaptive
from psa_amd.phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
from psa_amd.simulation import run_single_simulation_adaptive
from psa_amd.sweep import rk4_sweep, rk45_sweep
from psa_amd.yaman_model import rhs_yaman_simplified

pytestmark = pytest.mark.gpu

G18 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G18.npz"))
CASES = ["g1_r6", "g1_r9", "g1_r11", "sw", "zero", "g9"]
P_C2 = np.array([0.5, 0.5, 1e-5, 1e-5])


def case(name):
    return {k[len(name) + 1:]: G18[k] for k in G18.files if k.startswith(name + "_")}


def tol_of(g):
    return AdaptiveConfig(rtol=float(g["rtol"]), atol=float(g["atol"]), max_steps=int(g["max_steps"]))


def amp_bound(n_acc, status=0):
    """Bound on |A - A_ref| / max_j |A_ref_j|: 1e-10, or 5e-15 per accepted step on the ~50 000-step G9 runs, where the
    RHS statements' different rounding accumulates (as in test_rk45_host); 1e-8 on the G9 runs that end at the step cap
    (100 000 attempts at gamma = 50..1000, recorded by the NumPy restatement: the two agree to ~3e-9 there)."""
    return np.where(np.asarray(status) == 2, 1e-8, np.maximum(1e-10, 5e-15 * np.asarray(n_acc)))


def rel_rows(got, want):
    """per point: max |got - want| / max_j |want_j| (largest wave of that point)"""
    return np.max(np.abs(got - want), axis=-1) / np.max(np.abs(want), axis=-1)


@pytest.mark.parametrize("name", CASES)
def test_g18_through_rk45_sweep(name):
    g = case(name)
    db = np.atleast_1d(g["dbeta"])
    n_out = int(g["n_out"]) if "n_out" in g else 0
    r = rk45_sweep(db, z_max=float(g["z_max"]), tol=tol_of(g), gamma=g["gamma"], alpha=float(g["alpha"]),
                   a0=np.sqrt(g["p_in"]).astype(complex), n_out=n_out)
    np.testing.assert_array_equal(r.n_accepted, g["n_accepted"])
    np.testing.assert_array_equal(r.n_rejected, g["n_rejected"])
    np.testing.assert_array_equal(r.status, g["status"])
    ok = g["status"] == 0
    np.testing.assert_array_equal(r.z_end[ok], g["z_end"][ok])
    np.testing.assert_allclose(r.z_end[~ok], g["z_end"][~ok], rtol=1e-9)
    assert np.all(rel_rows(r.a_end, g["a_end"]) < amp_bound(g["n_accepted"], g["status"]))
    p_top = np.max(np.abs(g["a_end"]) ** 2, axis=1)
    assert np.all(np.abs(r.p_max - g["p_max"]) / p_top < 2 * amp_bound(g["n_accepted"], g["status"]))
    p0 = float(g["p_in"][2])
    if p0 > 0.0:   # example_zero_signal has no signal and no gain
        gain = r.gain(p0)
        np.testing.assert_array_equal(np.isnan(gain), ~ok)
        want = 10 * np.log10(g["p_max"][ok] / p0)
        # 5e-9 dB; on the ~50 000-step G9 runs what the p_max bound above allows on the signal (10/ln 10 * relative
        # power error), since the two RHS statements' rounding accumulates there
        gtol = np.full(ok.shape, 5e-9)
        if name == "g9":
            gtol = np.maximum(gtol, 4.35 * 2 * amp_bound(g["n_accepted"], g["status"]) * p_top / g["p_max"])
        assert np.all(np.abs(gain[ok] - want) < gtol[ok])
    if n_out:
        rows = g["rows"]
        assert np.max(np.abs(r.traj[0] - rows) / np.max(np.abs(rows), axis=0)) < 1e-10
        np.testing.assert_array_equal(r.z_out, np.linspace(0.0, float(g["z_max"]), n_out + 1))


def test_g18_through_run_single_simulation_adaptive():
    g = case("g1_r9")
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=float(g["dbeta"][0]))
    cfg = custom_simulation_config(z_max=float(g["z_max"]), dz=1.0, save_every=1)
    w0 = 2 * np.pi * 299792458.0 / 1.55e-6
    z, A = run_single_simulation_adaptive(cfg, tol=tol_of(g), gamma=float(g["gamma"]), alpha=float(g["alpha"]),
                                          omega=np.full(4, w0), p_in=g["p_in"], phase_matching_cfg=pm)
    rows = g["rows"]
    np.testing.assert_array_equal(z, np.linspace(0.0, 1000.0, 1001))
    assert A.shape == rows.shape
    assert np.max(np.abs(A - rows) / np.max(np.abs(rows), axis=0)) < 1e-10
    # a coarser sampling grid: every 10th row of the same run
    z10, A10 = run_single_simulation_adaptive(custom_simulation_config(z_max=1000.0, dz=1.0, save_every=10),
                                              tol=tol_of(g), gamma=float(g["gamma"]), alpha=float(g["alpha"]),
                                              omega=np.full(4, w0), p_in=g["p_in"], phase_matching_cfg=pm)
    np.testing.assert_array_equal(z10, z[::10])
    assert np.max(np.abs(A10 - rows[::10]) / np.max(np.abs(rows), axis=0)) < 1e-10


@pytest.mark.parametrize("z_max,dz,save_every,unit", [(10.0, 1.0, 3, "m"), (1000.0, 1.0, 7, "m"), (123.4, 0.1, 4, "m"),
                                                       (0.7, 0.01, 5, "m"), (0.5, 1e-4, 3, "km"), (1000.0, 1.0, 10, "m")])
def test_run_single_simulation_adaptive_rows_lie_on_the_fixed_step_grid(z_max, dz, save_every, unit):
    """z_out equals run_single_simulation's bit for bit, also where save_every does not divide n_steps (the last row short
    of z_max) and where the two linspace forms would differ by an ulp; the rows agree with the fixed-step run's to its
    accuracy."""
    from psa_amd.simulation import run_single_simulation
    w0 = 2 * np.pi * 299792458.0 / 1.55e-6
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.013)
    g = 0.0115 * (1000.0 if unit == "km" else 1.0)
    kw = dict(gamma=g, alpha=0.0, omega=np.full(4, w0), p_in=P_C2, phase_matching_cfg=pm, length_unit=unit)
    cfg = custom_simulation_config(z_max=z_max, dz=dz, save_every=save_every)
    z4, A4 = run_single_simulation(cfg, **kw)
    z5, A5 = run_single_simulation_adaptive(cfg, tol=AdaptiveConfig(rtol=1e-10, atol=1e-13), **kw)
    np.testing.assert_array_equal(z5, z4)
    assert A5.shape == A4.shape
    # RK4 at dz (<= 3.3e-7 from converged at dz = 1 m on these inputs) against RK45 at rtol 1e-10
    assert np.max(np.abs(A5 - A4) / np.max(np.abs(A4), axis=0)) < 1e-6


def test_run_single_simulation_adaptive_lengths_follow_length_unit():
    """h_max and first_step are in length_unit: the same fibre in km and in m takes the same steps."""
    w0 = 2 * np.pi * 299792458.0 / 1.55e-6
    pm_m = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.013)
    pm_km = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=13.0)
    base = dict(alpha=0.0, omega=np.full(4, w0), p_in=P_C2)
    tol_m = AdaptiveConfig(rtol=1e-9, h_max=2.0, first_step=0.5)
    tol_km = AdaptiveConfig(rtol=1e-9, h_max=2e-3, first_step=5e-4)
    z_m, A_m = run_single_simulation_adaptive(custom_simulation_config(z_max=1000.0, dz=10.0), tol=tol_m, gamma=0.0115,
                                              phase_matching_cfg=pm_m, **base)
    z_k, A_k = run_single_simulation_adaptive(custom_simulation_config(z_max=1.0, dz=0.01), tol=tol_km, gamma=11.5,
                                              phase_matching_cfg=pm_km, length_unit="km", return_length_unit="m", **base)
    np.testing.assert_allclose(z_k, z_m, rtol=1e-15, atol=1e-12)
    assert np.max(np.abs(A_k - A_m) / np.max(np.abs(A_m), axis=0)) < 1e-12
    # an h_max read as metres in the km run would allow 1000x longer steps: the results would differ at ~1e-9, not 1e-12
    loose = run_single_simulation_adaptive(custom_simulation_config(z_max=1.0, dz=0.01), tol=tol_m, gamma=11.5,
                                           phase_matching_cfg=pm_km, length_unit="km", **base)[1]
    assert np.max(np.abs(loose - A_m) / np.max(np.abs(A_m), axis=0)) > 1e-12


def test_run_single_simulation_adaptive_failures():
    w0 = 2 * np.pi * 299792458.0 / 1.55e-6
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.01)
    kw = dict(gamma=1000.0, alpha=0.0, omega=np.full(4, w0), p_in=P_C2, phase_matching_cfg=pm)
    with pytest.raises(RuntimeError, match="max_steps"):
        run_single_simulation_adaptive(custom_simulation_config(z_max=100.0, dz=0.1), tol=AdaptiveConfig(max_steps=2000),
                                       **kw)


@pytest.mark.parametrize("name", ["g1_r6", "g1_r9", "g1_r11", "zero"])
def test_g18_through_integrate_adaptive(name):
    g = case(name)
    params = SimpleNamespace(fiber=SimpleNamespace(gamma_W_m=float(g["gamma"]), alpha_1_m=float(g["alpha"])),
                             cache=SimpleNamespace(delta_beta_1_m=float(g["dbeta"][0])))
    n_out = int(g["n_out"]) if "n_out" in g else 10
    z, rows, info = integrate_adaptive(rhs_yaman_simplified, float(g["z_max"]), np.sqrt(g["p_in"]).astype(complex),
                                       params, tol=tol_of(g), n_out=n_out)
    assert (info["n_accepted"], info["n_rejected"], info["status"]) == \
        (int(g["n_accepted"][0]), int(g["n_rejected"][0]), int(g["status"][0]))
    assert info["z_end"] == float(g["z_end"][0])
    assert rel_rows(info["y_end"], g["a_end"][0]) < 1e-10
    if "rows" in g:
        assert np.max(np.abs(rows - g["rows"]) / np.max(np.abs(g["rows"]), axis=0)) < 1e-10


def _compare_to_numpy(r, ref, rtol):
    same = (r.n_accepted == ref["n_accepted"]) & (r.n_rejected == ref["n_rejected"])
    assert np.mean(same) >= 0.95, np.mean(same)
    err = rel_rows(r.a_end, ref["a_end"])
    assert np.all(err[same] < 1e-10), np.max(err[same])
    assert np.all(err < 100 * rtol), np.max(err)
    assert np.all(r.status == 0) and np.all(ref["status"] == 0)


def test_random_sweep_against_numpy_restatement():
    n, rtol, alpha = 4096, 1e-9, 1.15e-4
    db, gamma, a0, _ = _random_points(n, 20261016)
    tol = AdaptiveConfig(rtol=rtol, atol=1e-12)
    r = rk45_sweep(db, z_max=1000.0, tol=tol, gamma=gamma, alpha=alpha, a0=a0)
    ref = rk45_np.rk45(rk45_np.rhs4(db, gamma, alpha), a0.T, 1000.0, rtol=rtol, atol=1e-12)
    _compare_to_numpy(r, ref, rtol)


def test_random_six_wave_sweep_against_numpy_restatement():
    n, rtol, alpha = 64, 1e-9, 1.15e-4
    db, gamma, a0, db2 = _random_points(n, 6, six=True)
    tol = AdaptiveConfig(rtol=rtol, atol=1e-12)
    r = rk45_sweep(db, z_max=500.0, tol=tol, gamma=gamma, alpha=alpha, a0=a0, dbeta2=db2)
    ref = rk45_np.rk45(rk45_np.rhs6(db, db2, gamma, alpha), a0.T, 500.0, rtol=rtol, atol=1e-12)
    _compare_to_numpy(r, ref, rtol)


def _config2(n):
    """BASELINE config-2 inputs (the figures of DESIGN.md 3.7): dbeta = linspace(-0.05, 0.05), gamma 0.0115, P_C2."""
    return np.linspace(-0.05, 0.05, n), np.full(n, 0.0115), np.repeat(np.sqrt(P_C2).astype(complex)[None, :], n, axis=0)


ARBITER_POINTS = 17


def _independent_arbiter(db, gamma, a0, n, n_out=1):
    """The global error's second arbiter, none of the project's GPU code: 17 of the points spread over the sweep through the
    compiled plain RK4 in 80 bits (oracle/plain_rk4.py) at the 4e5 steps of the GPU one, rows at the dense grid.
    -> (the points picked, its rows (17, n_out + 1, 4) as complex128)."""
    import plain_rk4
    pick = np.linspace(0, n - 1, ARBITER_POINTS).astype(int)
    ld = plain_rk4.integrate("pairs", a0[pick], db[pick], z_max=1000.0, n=400_000, save_every=400_000 // n_out,
                             gamma=gamma[pick], alpha=1.15e-4, precision="ld", want_rows=True)
    return pick, ld["rows"].astype(np.complex128)


def test_accuracy_against_converged_rk4():
    # rtol bounds the local error per step, not the global one: on config-2 inputs the global error stays within
    # 100 * rtol; at gamma * P * L ~ 20 rad (the random set above) it reaches ~2e-7 at rtol 1e-9
    n, rtol = 256, 1e-9
    db, gamma, a0 = _config2(n)
    r = rk45_sweep(db, z_max=1000.0, tol=AdaptiveConfig(rtol=rtol), gamma=gamma, alpha=1.15e-4, a0=a0)
    truth = rk4_sweep(db, z_max=1000.0, n_steps=400_000, save_every=400_000, gamma=gamma, alpha=1.15e-4, a0=a0)
    assert np.all(r.status == 0)
    assert np.max(rel_rows(r.a_end, truth.a_end)) < 100 * rtol
    pick, rows = _independent_arbiter(db, gamma, a0, n)
    assert np.max(rel_rows(r.a_end[pick], rows[:, -1])) < 100 * rtol


def test_lane_independence():
    g1 = case("g1_r9")
    tol = AdaptiveConfig(rtol=1e-9, atol=1e-12, max_steps=20_000)
    a_g1 = np.sqrt(g1["p_in"]).astype(complex)
    alone = rk45_sweep([float(g1["dbeta"][0])], z_max=1000.0, tol=tol, gamma=float(g1["gamma"]),
                       alpha=float(g1["alpha"]), a0=a_g1, n_out=50)
    # 64 neighbours of one wave: G9's gamma = 1000 (runs into max_steps), a NaN a0 (status 1), more G1 copies
    n = 64
    gamma = np.full(n, float(g1["gamma"]))
    a0 = np.repeat(a_g1[None, :], n, axis=0)
    gamma[1::3] = 1000.0
    a0[2::3, 2] = np.nan
    db = np.full(n, float(g1["dbeta"][0]))
    mixed = rk45_sweep(db, z_max=1000.0, tol=tol, gamma=gamma, alpha=np.full(n, float(g1["alpha"])), a0=a0, n_out=50)
    for k in range(0, n, 3):   # every G1 copy equals the lone run bit for bit
        for field in ("a_end", "p_end", "p_max", "status", "z_end", "n_accepted", "n_rejected", "traj"):
            np.testing.assert_array_equal(getattr(mixed, field)[k], getattr(alone, field)[0], err_msg=field)
    assert np.all(mixed.status[1::3] == 2) and np.all(mixed.status[2::3] == 1)
    assert np.all(mixed.n_accepted[2::3] == 0) and np.all(mixed.z_end[2::3] == 0.0)
    assert np.all(np.isnan(mixed.traj[2::3, 1:]))


def test_failure_statuses_and_gain():
    n = 32
    gamma = np.where(np.arange(n) % 4 == 0, 1000.0, 0.0115)
    tol = AdaptiveConfig(rtol=1e-9, max_steps=3000)
    r = rk45_sweep(np.linspace(-0.05, 0.05, n), z_max=1000.0, tol=tol, gamma=gamma, alpha=1.15e-4, a0=np.sqrt(P_C2))
    bad = gamma == 1000.0
    assert np.all(r.status[bad] == 2) and np.all(r.status[~bad] == 0)
    assert np.all(r.z_end[bad] < 1000.0) and np.all(r.z_end[~bad] == 1000.0)
    assert np.all(r.n_accepted[bad] + r.n_rejected[bad] == 3000)
    np.testing.assert_array_equal(r.first_bad_step, np.where(bad, r.n_accepted, -1))
    gain, best, best_gain, n_finite = r.summary(1e-5)
    np.testing.assert_array_equal(np.isnan(gain), bad)
    assert n_finite == int((~bad).sum()) and best_gain == np.nanmax(gain) and gain[best] == best_gain


def test_dev_form_equals_host_form_and_replays_from_a_graph():
    import torch
    dev = torch.device("cuda", 0)
    n, nw, n_out = 300, 4, 20
    db, gamma, a0, _ = _random_points(n, 77)
    alpha = np.full(n, 1.15e-4)
    tol = dict(z_max=800.0, rtol=1e-8, atol=1e-12, h_max=np.inf, first_step=0.0, max_steps=100_000)
    host = nat.rk45_sweep_host(db, gamma=gamma, alpha=alpha, a0=a0, n_out=n_out, **tol)
    f64 = dict(dtype=torch.float64, device=dev)
    d_db, d_g, d_a = torch.tensor(db, **f64), torch.tensor(gamma, **f64), torch.tensor(alpha, **f64)
    d_a0 = torch.tensor(np.ascontiguousarray(a0.view(np.float64).T), **f64)
    d_aend = torch.empty((2 * nw, n), **f64)
    d_pe, d_pm, d_ze = (torch.empty(n, **f64) for _ in range(3))
    d_st = torch.empty(n, dtype=torch.int32, device=dev)
    d_na, d_nr = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    d_tr = torch.empty((n_out + 1, nw, n, 2), **f64)

    def launch():
        nat.rk45_sweep_device(stream=torch.cuda.current_stream().cuda_stream, n_waves=nw, n_points=n, n_out=n_out,
                              d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(), d_alpha=d_a.data_ptr(),
                              d_a0_soa=d_a0.data_ptr(), flags=0, d_a_end_soa=d_aend.data_ptr(), d_p_end=d_pe.data_ptr(),
                              d_p_max=d_pm.data_ptr(), d_status=d_st.data_ptr(), d_z_end=d_ze.data_ptr(),
                              d_n_accepted=d_na.data_ptr(), d_n_rejected=d_nr.data_ptr(), d_traj_soa=d_tr.data_ptr(),
                              **tol)

    def check(ref):
        torch.cuda.synchronize()
        assert np.array_equal(np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128), ref["a_end"])
        for t, k in ((d_pe, "p_end"), (d_pm, "p_max"), (d_ze, "z_end"), (d_st, "status"), (d_na, "n_accepted"),
                     (d_nr, "n_rejected")):
            assert np.array_equal(t.cpu().numpy(), ref[k]), k
        traj = np.ascontiguousarray(d_tr.cpu().numpy().transpose(2, 0, 1, 3)).view(np.complex128)[..., 0]
        assert np.array_equal(traj, ref["traj"])

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch()
    side.synchronize()
    check(host)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    db2 = np.random.default_rng(5).uniform(-0.1, 0.1, n)
    d_db.copy_(torch.tensor(db2, **f64))
    for t in (d_aend, d_pe, d_pm, d_ze, d_tr):
        t.zero_()
    graph.replay()
    check(nat.rk45_sweep_host(db2, gamma=gamma, alpha=alpha, a0=a0, n_out=n_out, **tol))


def test_dense_rows():
    n, n_out, rtol = 64, 250, 1e-9
    db, gamma, a0 = _config2(n)
    r = rk45_sweep(db, z_max=1000.0, tol=AdaptiveConfig(rtol=rtol), gamma=gamma, alpha=1.15e-4, a0=a0, n_out=n_out)
    np.testing.assert_array_equal(r.traj[:, 0], a0)
    assert np.max(rel_rows(r.traj[:, -1], r.a_end)) < 1e-13
    fixed = rk4_sweep(db, z_max=1000.0, n_steps=400_000, save_every=400_000 // n_out, gamma=gamma, alpha=1.15e-4, a0=a0,
                      want_traj=True)
    assert fixed.traj.shape == r.traj.shape
    scale = np.max(np.abs(fixed.traj), axis=2, keepdims=True)
    assert np.max(np.abs(r.traj - fixed.traj) / scale) < 100 * rtol
    pick, rows = _independent_arbiter(db, gamma, a0, n, n_out)
    assert rows.shape == r.traj[pick].shape
    assert np.max(np.abs(r.traj[pick] - rows) / np.max(np.abs(rows), axis=2, keepdims=True)) < 100 * rtol


def test_lossless_path_equals_lossy_instantiation():
    n = 128
    db, gamma, a0, _ = _random_points(n, 3)
    tol = AdaptiveConfig(rtol=1e-9)
    lossless = rk45_sweep(db, z_max=1000.0, tol=tol, gamma=gamma, alpha=0.0, a0=a0, n_out=10)          # LOSSLESS (auto)
    lossy = rk45_sweep(db, z_max=1000.0, tol=tol, gamma=gamma, alpha=np.zeros(n), a0=a0, n_out=10)     # per-point alpha
    for field in ("a_end", "p_end", "p_max", "status", "z_end", "n_accepted", "n_rejected", "traj"):
        np.testing.assert_array_equal(getattr(lossless, field), getattr(lossy, field), err_msg=field)
    six_db, six_g, six_a0, six_db2 = _random_points(16, 4, six=True)
    a = rk45_sweep(six_db, z_max=300.0, tol=tol, gamma=six_g, alpha=0.0, a0=six_a0, dbeta2=six_db2)
    b = rk45_sweep(six_db, z_max=300.0, tol=tol, gamma=six_g, alpha=np.zeros(16), a0=six_a0, dbeta2=six_db2)
    np.testing.assert_array_equal(a.a_end, b.a_end)
    np.testing.assert_array_equal(a.n_accepted, b.n_accepted)
