"""Multi-line ("comb") fibre chains on the GPU (psa_rk4_comb_chain_f64, sweep.rk4_chain_comb,
simulation.run_concatenated_comb_simulation, scan_mismtach.scan_comb_copier_psa_phase) against the NumPy restatement
tests/comb_chain_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest line):

* one span is psa_rk4_comb_f64 bit for bit, with and without rows, M = 3 and 12;
* one fibre cut into 2, 3 and 7 spans with identity transfers is the unsplit sweep, M = 4 and 12;
* a lossy three-span chain with per-point kappa (N, M), gamma, alpha, a per-point and a broadcast transfer, M = 3, 7, 12: 300
  points cross a 256-thread epilogue block;
* spans of 1, 63, 64, 65 and 130 steps in one chain (the kernel re-seeds its phases every 64 steps);
* M = 3 against rk4_chain_single_pump at 1e-10;
* a failure in span 2 is reported at the chain's step index, its neighbours untouched, a third span changes nothing;
* the `_dev` entry on a caller's workspace of exactly the stated size and padded trajectory rows, bit-equal to the host form;
* devices=[0, 0] equals one device; the span driver against the unsplit single run; the phase-scan driver at M = 3 against
  the single-pump closed form and a direct chain call."""
import functools

import numpy as np
import pytest

import comb_chain_np as chain_np
import psa_amd._native as nat
import single_pump_chain_np
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach, simulation
from psa_amd.frequency_plan import omega_from_lambda
from psa_amd.sweep import FibreSpan, rk4_chain_comb, rk4_chain_single_pump, rk4_sweep_comb

pytestmark = pytest.mark.gpu

KEYS = ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")


def wave_err(got, ref):
    """max |got - ref| over the largest line of the point (amplitudes (N, ..., M) complex)."""
    ref = np.asarray(ref)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return float(np.max(np.abs(np.asarray(got) - ref) / scale))


def power_err(got, ref):
    """The same bar on a power summary (N, M): the lines' moduli sqrt(P_m) against the point's largest."""
    return wave_err(np.sqrt(np.asarray(got)).astype(complex), np.sqrt(np.asarray(ref)).astype(complex))


def _fibre(spans):
    return [FibreSpan(L, n_steps=n, dbeta=kp, gamma=g, alpha=al) for L, n, kp, g, al in spans]


def _strided(rows, z_out, steps, se):
    """Rows of a chain saved every ``se`` steps, out of the rows saved at every step."""
    offs = np.concatenate([[0], np.cumsum(np.asarray(steps) + 1)[:-1]])
    idx = np.concatenate([o + np.arange(0, s - s % se + 1, se) for o, s in zip(offs, steps)])
    return rows[:, idx], z_out[idx]


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


# ---- identity split -------------------------------------------------------------------------------------------------------
def _split(n, cuts, se):
    steps = np.full(cuts, (n // se // cuts) * se)
    steps[-1] = n - steps[:-1].sum()
    return [int(s) for s in steps]


def _rows(steps, se):
    offs = np.concatenate([[0], np.cumsum(steps)[:-1]])
    return np.concatenate([o // se + np.arange(s // se + 1) for o, s in zip(offs, steps)])


@functools.lru_cache(maxsize=None)
def _unsplit(M):
    n_pts, n, L, se = 33, 1400, 700.0, 10
    rng = np.random.default_rng(2 + M)
    kp, a0 = chain_np.random_kappa(rng, n_pts, M), chain_np.random_a0(rng, n_pts, M)
    gamma, alpha = chain_np.GAMMA * rng.uniform(0.9, 1.1, n_pts), 1.15e-4 * rng.uniform(0.5, 1.5, n_pts)
    whole = rk4_sweep_comb(kp, z_max=L, n_steps=n, save_every=se, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    return kp, a0, gamma, alpha, whole


@pytest.mark.parametrize("cuts", [2, 3, 7])
@pytest.mark.parametrize("M", [4, 12])
def test_identity_split_equals_the_unsplit_run(M, cuts):
    n_pts, n, L, se = 33, 1400, 700.0, 10
    kp, a0, gamma, alpha, whole = _unsplit(M)
    steps = _split(n, cuts, se)
    spans = [FibreSpan(L * s / n, n_steps=s, dbeta=kp, gamma=gamma, alpha=alpha) for s in steps]
    got = rk4_chain_comb(spans, a0=a0, transfers=[np.ones(M)] * (cuts - 1), save_every=se, want_traj=True)
    assert got.traj.shape == (n_pts, sum(s // se + 1 for s in steps), M) and got.n_steps == n
    np.testing.assert_allclose(got.z_out, np.linspace(0, L, n + 1)[::se][_rows(steps, se)], rtol=1e-12, atol=1e-9)
    errs = dict(a_end=wave_err(got.a_end, whole.a_end), p_wave_end=power_err(got.p_wave_end, whole.p_wave_end),
                p_wave_max=power_err(got.p_wave_max, whole.p_wave_max), rows=wave_err(got.traj, whole.traj[:, _rows(steps, se)]))
    print(f"M = {M}, {cuts} spans against the unsplit sweep: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL_F64
    assert np.all(got.first_bad_step == -1)
    # without the trajectory the summaries are the same numbers
    lean = rk4_chain_comb(spans, a0=a0, save_every=se)
    for key in KEYS:
        assert np.array_equal(getattr(lean, key), getattr(got, key)), key
    assert lean.traj is None


# ---- the lossy three-span chain -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lossy_reference(M):
    """300 points through the restatement once, every step saved; any save stride is read off the rows."""
    case = chain_np.lossy_case(300, M, steps=(120, 200, 80))
    ref = chain_np.chain(*case, 1)
    assert (ref["first_bad_step"] == -1).all()
    return case, ref["rows"], ref["z_out"]


@pytest.mark.parametrize("save_every", [1, 20])
@pytest.mark.parametrize("M", [3, 7, 12])
def test_lossy_chain_with_transfers_against_the_restatement(M, save_every):
    (a0, spans, transfers), rows, z_all = _lossy_reference(M)
    want, z_want = _strided(rows, z_all, [n for _, n, *_ in spans], save_every)
    got = rk4_chain_comb(_fibre(spans), a0=a0, transfers=transfers, save_every=save_every, want_traj=True)
    assert got.traj.shape == want.shape
    errs = (wave_err(got.traj, want), wave_err(got.a_end, want[:, -1]), power_err(got.p_wave_end, np.abs(want[:, -1]) ** 2),
            power_err(got.p_wave_max, np.max(np.abs(want) ** 2, axis=1)))
    print(f"lossy 3-span chain, M = {M}, 300 points, save_every={save_every}: rows {errs[0]:.2e} a_end {errs[1]:.2e} "
          f"p_wave_end {errs[2]:.2e} p_wave_max {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    np.testing.assert_allclose(got.z_out, z_want, rtol=1e-14, atol=0.0)
    assert np.all(got.first_bad_step == -1) and np.array_equal(got.traj[:, -1], got.a_end)
    assert np.array_equal(got.row_offsets, np.concatenate([[0], np.cumsum([n // save_every + 1 for _, n, *_ in spans])]))


def test_loop_edges_in_one_chain():
    """Spans of 1, 63, 64, 65 and 130 steps, every step saved, per-point transfers between them."""
    N, M, steps = 70, 4, (1, 63, 64, 65, 130)
    rng = np.random.default_rng(5)
    a0 = chain_np.random_a0(rng, N, M)
    G = chain_np.GAMMA
    spans = [(2.0 * n, n, chain_np.random_kappa(rng, N, M), G * rng.uniform(0.9, 1.3, N), 1.15e-4 * rng.uniform(0.0, 2.0, N))
             for n in steps]
    transfers = [chain_np.mid_stage(rng.uniform(-2, 1, (N, M)), rng.uniform(-np.pi, np.pi, (N, M))) for _ in steps[1:]]
    ref = chain_np.chain(a0, spans, transfers, 1)
    got = rk4_chain_comb(_fibre(spans), a0=a0, transfers=transfers, save_every=1, want_traj=True)
    errs = (wave_err(got.traj, ref["rows"]), wave_err(got.a_end, ref["a_end"]), power_err(got.p_wave_max, ref["p_wave_max"]))
    print(f"loop edges: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_max {errs[2]:.2e}")
    assert got.traj.shape == (N, sum(steps) + len(steps), M) and max(errs) < RTOL_F64 and np.all(got.first_bad_step == -1)


# ---- three lines are the single-pump chain --------------------------------------------------------------------------------
def test_three_lines_against_rk4_chain_single_pump():
    """The lossy three-span case of the single-pump chain (300 points, 120 + 200 + 80 steps) on lines [s, p, i], every span's
    dbeta split at random into kappa_0 + kappa_2 - 2 kappa_1: the two kernels order their products differently, so they agree
    to rounding, 1e-10 of the point's largest wave."""
    case = single_pump_chain_np.lossy_case(300, steps=(120, 200, 80))
    a0, spans, transfers = chain_np.from_single_pump(case, np.random.default_rng(6))
    kw = dict(save_every=20, want_traj=True)
    got = rk4_chain_comb(_fibre(spans), a0=a0, transfers=transfers, **kw)
    ref = rk4_chain_single_pump(_fibre(case[1]), a0=case[0], transfers=case[2], **kw)
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
    got = rk4_chain_comb(_fibre(spans), a0=a0, transfers=[np.ones(4)], save_every=10)
    np.testing.assert_array_equal(got.first_bad_step, ref["first_bad_step"])
    ok = [0, 2, 4]
    assert np.all(np.isnan(got.p_wave_max[[1, 3]])) and np.all(np.isfinite(got.p_wave_max[ok]))
    g = got.line_gain(np.abs(a0) ** 2, mode="max")
    assert np.all(np.isnan(g[[1, 3]])) and np.all(np.isfinite(g[ok]))
    errs = (wave_err(got.a_end[ok], ref["a_end"][ok]), power_err(got.p_wave_end[ok], ref["p_wave_end"][ok]),
            power_err(got.p_wave_max[ok], ref["p_wave_max"][ok]))
    assert max(errs) < RTOL_F64
    third = (10.0, 100, spans[0][2], chain_np.GAMMA, 0.0)
    more = rk4_chain_comb(_fibre(spans + [third]), a0=a0, transfers=[np.ones(4)] * 2, save_every=10)
    np.testing.assert_array_equal(more.first_bad_step, ref["first_bad_step"])
    ref3 = chain_np.chain(a0, spans + [third], [np.ones(4)] * 2, 10)
    assert wave_err(more.a_end[ok], ref3["a_end"][ok]) < RTOL_F64 and power_err(more.p_wave_max[ok], ref3["p_wave_max"][ok]) < RTOL_F64


# ---- the _dev entry -------------------------------------------------------------------------------------------------------
def _device_chain(torch, a0, spans, transfers, *, save_every, flags, ld):
    """psa_rk4_comb_chain_f64_dev on torch buffers with a workspace of exactly the stated size (and a guard behind it) -> the
    host entry's dictionary, the trajectory's padding and the guard."""
    dev = torch.device("cuda:0")
    N, M, S = a0.shape[0], a0.shape[1], len(spans)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_kp = t(np.stack([sp[2] for sp in spans]).transpose(0, 2, 1))                       # (S, M, N)
    d_g, d_al = (t(np.stack([sp[k] for sp in spans])) for k in (3, 4))
    d_a0 = t(a0.view(np.float64).reshape(N, 2 * M).T)
    tr = np.stack([np.broadcast_to(x, (N, M)) for x in transfers])                       # (S-1, N, M)
    d_tr = t(np.ascontiguousarray(tr).view(np.float64).reshape(S - 1, N, 2 * M).transpose(0, 2, 1))
    d_aend = torch.empty((2 * M, N), dtype=torch.float64, device=dev)
    d_we, d_wm = torch.empty((M, N), dtype=torch.float64, device=dev), torch.empty((M, N), dtype=torch.float64, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    steps = [sp[1] for sp in spans]
    rows = sum(n // save_every + 1 for n in steps)
    d_traj = torch.full((rows, M, ld, 2), -7.0, dtype=torch.float64, device=dev)
    ws_bytes = nat.comb_chain_workspace_bytes(M, N)
    d_ws = torch.full((ws_bytes + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    nat.comb_chain_device(stream=torch.cuda.current_stream().cuda_stream, n_lines=M, n_points=N, n_steps=steps,
                          seg_len=[sp[0] for sp in spans], save_every=save_every, d_kappa_soa=d_kp.data_ptr(),
                          d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(),
                          d_transfer_soa=d_tr.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                          d_p_wave_end_soa=d_we.data_ptr(), d_p_wave_max_soa=d_wm.data_ptr(),
                          d_first_bad=d_bad.data_ptr(), d_traj_soa=d_traj.data_ptr(), d_workspace=d_ws.data_ptr())
    torch.cuda.synchronize()
    full = d_traj.cpu().numpy()                                                          # [rows][M][ld][2]
    return dict(a_end=np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128), p_wave_end=d_we.cpu().numpy().T,
                p_wave_max=d_wm.cpu().numpy().T, first_bad_step=d_bad.cpu().numpy(),
                traj=np.ascontiguousarray(full[:, :, :N].transpose(2, 0, 1, 3)).view(np.complex128)[..., 0],
                pad=full[:, :, N:], guard=d_ws[ws_bytes:].cpu().numpy())


@pytest.mark.parametrize("N,M,steps,lengths", [(300, 4, (60, 100, 40), (300.0, 500.0, 200.0)), (131072, 3, (20, 20), (10.0, 10.0))],
                         ids=["300", "131072-padded"])
def test_device_entry_equals_the_host_entry_bit_for_bit(N, M, steps, lengths):
    """PSA_OPT_TRAJ_LD on the `_dev` form: ld = psa_traj_ld(N, 8), which is N for 300 points and N + 272 for 131 072.  The
    padding and the bytes behind the workspace are never written; a handful of the padded case's points also go against
    the restatement, which an epilogue that ignored the leading dimension would miss."""
    import torch
    se = 20 if N == 300 else 10
    ld = nat.traj_ld(N)
    assert ld == (N if N == 300 else N + 272)
    a0, spans, transfers = chain_np.lossy_case(N, M, steps=steps, lengths=lengths)
    transfers = transfers[:len(steps) - 1]
    case = (a0, spans, transfers)
    host = nat.comb_chain_host(np.stack([sp[2] for sp in spans]), n_steps=steps, seg_len=lengths, save_every=se,
                               gamma=np.stack([sp[3] for sp in spans]), alpha=np.stack([sp[4] for sp in spans]), a0=a0,
                               transfers=np.stack([np.broadcast_to(x, a0.shape) for x in transfers]), want_traj=True)
    got = _device_chain(torch, a0, spans, transfers, save_every=se, flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_TRAJ_LD,
                        ld=ld)
    for key in KEYS + ("traj",):
        assert np.array_equal(got[key], host[key]), key
    assert got["pad"].shape[2] == ld - N and np.all(got["pad"] == -7.0) and np.all(got["guard"] == 0x5A)
    idx = np.array([0, 1, 63, 64, 255, 256, N // 2, N - 2, N - 1])
    ref = chain_np.chain(*chain_np.subset(case, idx), se)
    assert wave_err(got["traj"][idx], ref["rows"]) < RTOL_F64 and power_err(got["p_wave_max"][idx], ref["p_wave_max"]) < RTOL_F64
    assert np.all(got["first_bad_step"] == -1)


# ---- devices and the span driver ------------------------------------------------------------------------------------------
def test_two_devices_equal_one():
    a0, spans, transfers = chain_np.lossy_case(41, 5, steps=(60, 100, 40))
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    one = rk4_chain_comb(_fibre(spans), **kw)
    two = rk4_chain_comb(_fibre(spans), devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (41, 4 + 6 + 3, 5)


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
    rows = _rows([600, 800], 10)
    assert Ac.shape == (61 + 81, 6) and A.shape == (141, 6)
    err = wave_err(Ac[None], A[rows][None])
    print(f"span driver against the single run: {err:.2e}")
    assert err < RTOL_F64
    np.testing.assert_allclose(zc, z[rows], rtol=1e-12, atol=1e-9)


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
