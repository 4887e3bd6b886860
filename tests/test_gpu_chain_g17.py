"""Fibre chains against the reference (tests/golden/G17.npz, written by gen_golden_chain.py from the reference's
run_single_simulation with the gauge applied between calls), and the device face of the chain:

* (a) a G8-like fibre whole and cut into 2 and 3 spans, (b) a lossy three-span chain with transfers -- through rk4_chain and
  run_concatenated_simulation -- and (c) a copier - mid-stage - PSA scan of 32 pump phases x 2 PSA dbeta through
  scan_copier_psa_phase: <= 1e-9 relative on amplitudes, <= 1e-9 relative on the gain in dB;
* psa_rk4_chain_f64_dev on caller-owned HBM buffers (per-point alpha, PSA_BCAST_TRANSFER, the caller's workspace) equals
  the host-buffer form bit for bit, also when captured into a graph and replayed on new inputs."""
import os

import numpy as np
import pytest

import psa_amd._native as nat
from psa_amd.config import custom_simulation_config
from psa_amd.phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
from psa_amd.scan_mismtach import scan_copier_psa_phase
from psa_amd.simulation import mid_stage, run_concatenated_simulation
from psa_amd.sweep import FibreSpan, rk4_chain

pytestmark = pytest.mark.gpu

G17 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G17.npz"))


def _col_rel(got, want):
    """max over rows of |got - want| / (max |want| of that wave), per point."""
    return float(np.max(np.abs(got - want) / np.max(np.abs(want), axis=-2, keepdims=True)))


@pytest.mark.parametrize("cuts", [1, 2, 3])
def test_g17_split_through_rk4_chain(cuts):
    g = G17
    se, dz = int(g["save_every"]), float(g["split_dz"])
    spans = [FibreSpan(s * dz, dz=dz, dbeta=g["split_dbeta"], gamma=float(g["split_gamma"]), alpha=float(g["split_alpha"]))
             for s in g[f"split{cuts}_steps"]]
    r = rk4_chain(spans, a0=np.sqrt(g["split_p_in"]).astype(complex), transfers=[np.ones(4)] * (cuts - 1),
                  save_every=se, want_traj=True)
    want = g[f"split{cuts}_A"]
    assert _col_rel(r.traj, want) < 1e-9
    assert _col_rel(r.a_end[:, None], want[:, -1:]) < 1e-9
    np.testing.assert_allclose(r.z_out, g[f"split{cuts}_z"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(r.p_max, np.max(np.abs(want[:, :, 2]) ** 2, axis=1), rtol=1e-9)


def _lossy_inputs():
    g = G17
    a0 = np.tile(np.sqrt(g["lossy_p_in"]).astype(complex), (g["lossy_phase_in"].size, 1))
    a0[:, 2] *= np.exp(1j * g["lossy_phase_in"])
    tr = [mid_stage(gd, ph) for gd, ph in zip(g["lossy_gain_db"], g["lossy_phase"])]
    return a0, tr


def test_g17_lossy_through_rk4_chain():
    g = G17
    a0, tr = _lossy_inputs()
    spans = [FibreSpan(L, dz=dz, dbeta=db, gamma=gm, alpha=al) for L, dz, db, gm, al in g["lossy_spans"]]
    r = rk4_chain(spans, a0=a0, transfers=tr, save_every=int(g["save_every"]), want_traj=True)
    assert _col_rel(r.traj, g["lossy_A"]) < 1e-9
    np.testing.assert_allclose(r.z_out, g["lossy_z"], rtol=1e-12, atol=1e-9)


def test_g17_lossy_through_run_concatenated_simulation():
    g = G17
    _, tr = _lossy_inputs()
    om = np.full(4, 2.0 * np.pi * 299792458.0 / 1.55e-6)
    spans = [dict(cfg=custom_simulation_config(z_max=float(L), dz=float(dz), save_every=int(g["save_every"])),
                  gamma=float(gm), alpha=float(al),
                  phase_matching_cfg=PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=float(db)))
             for L, dz, db, gm, al in g["lossy_spans"]]
    for i, phi in enumerate(g["lossy_phase_in"]):
        z, A = run_concatenated_simulation(spans, omega=om, p_in=g["lossy_p_in"], phase_in=[0.0, 0.0, phi, 0.0],
                                           transfers=tr)
        assert _col_rel(A, g["lossy_A"][i]) < 1e-9
        np.testing.assert_allclose(z, g["lossy_z"], rtol=1e-12, atol=1e-9)


def _scan(**over):
    g = G17
    L1, dz1, db1 = g["scan_copier"]
    L2, dz2 = g["scan_psa"]
    kw = dict(psa_cfg=custom_simulation_config(z_max=float(L2), dz=float(dz2), save_every=int(g["save_every"])),
              psa_delta_beta=g["scan_psa_dbeta"], gamma=float(g["scan_gamma"]), alpha=float(g["scan_alpha"]),
              p_in=g["scan_p_in"], copier_cfg=custom_simulation_config(z_max=float(L1), dz=float(dz1),
                                                                        save_every=int(g["save_every"])),
              copier_delta_beta=float(db1), mid_gain_db=g["scan_mid_gain_db"], phase=g["scan_phases"])
    kw.update(over)
    return scan_copier_psa_phase(**kw)


def test_g17_copier_psa_scan():
    g = G17
    p0 = float(g["scan_p_in"][2])
    out = _scan(gain_mode="max")
    want_max = 10 * np.log10(g["scan_p_sig_max"] / p0)
    assert out["gain"].shape == (32, 2)
    assert np.max(np.abs(out["gain"] - want_max) / np.abs(want_max)) < 1e-9
    assert abs(out["gain_max_db"] - want_max.max()) <= 1e-9 * abs(want_max.max())
    assert abs(out["extinction_db"] - (want_max.max() - want_max.min())) <= 1e-9 * abs(want_max.max())
    a_end = out["result"].a_end.reshape(32, 2, 4)
    assert np.max(np.abs(a_end - g["scan_A_end"]) / np.max(np.abs(g["scan_A_end"]), axis=(0, 1))) < 1e-9
    end = _scan(gain_mode="end", gain_unit="linear")
    want_end = np.abs(g["scan_A_end"][:, :, 2]) ** 2 / p0
    assert np.max(np.abs(end["gain"] / want_end - 1.0)) < 1e-9
    two = _scan(gain_mode="max", devices=[0, 0])
    assert np.array_equal(two["gain"], out["gain"])


def test_copier_psa_scan_nan_rule():
    """A PSA span past the RK4 stability edge: every point's gain is NaN (scan_mismtach.py:391-392), so are the extremes."""
    out = _scan(gamma=300.0, copier_gamma=float(G17["scan_gamma"]))
    assert np.all(np.isnan(out["gain"])) and np.isnan(out["gain_max_db"]) and np.isnan(out["extinction_db"])
    assert np.all(out["result"].first_bad_step > int(G17["scan_copier"][0] / G17["scan_copier"][1]))


def test_dev_form_equals_host_form_and_replays_from_a_graph():
    import torch
    dev = torch.device("cuda", 0)
    S, N, nw, se = 3, 300, 4, 10
    steps, lens = np.array([200, 300, 100]), np.array([100.0, 150.0, 50.0])
    rng = np.random.default_rng(3)
    dbeta = rng.uniform(-0.03, 0.03, (S, N))
    gamma = np.array([0.0115, 0.02, 0.009])
    alpha = np.stack([np.full(N, 1.2e-4), np.full(N, 3e-5), rng.uniform(0, 2e-4, N)])
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-6]).astype(complex), (N, 1)) * np.exp(1j * rng.uniform(0, 1, (N, 1)))
    tr = np.stack([mid_stage((-1.0, -1.0, 0.0, -3.0), (0.2, 0.1, 0.0, 0.0)), mid_stage((0.0, 0.0, 1.0, 0.0), 0.3)])
    host = nat.chain_host(dbeta, n_steps=steps, seg_len=lens, save_every=se, gamma=gamma, alpha=alpha, a0=a0, transfers=tr)

    f64 = dict(dtype=torch.float64, device=dev)
    d_db, d_g, d_a = torch.tensor(dbeta, **f64), torch.tensor(gamma, **f64), torch.tensor(alpha, **f64)
    d_a0 = torch.tensor(np.ascontiguousarray(a0.view(np.float64).T), **f64)          # SoA [2*nw][N]
    d_tr = torch.tensor(tr.view(np.float64), **f64)                                  # [S-1][2*nw]
    d_aend = torch.empty((2 * nw, N), **f64)
    d_pe, d_pm = torch.empty(N, **f64), torch.empty(N, **f64)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    d_ws = torch.empty(nat.chain_workspace_bytes(nw, N), dtype=torch.uint8, device=dev)
    flags = nat.BCAST_GAMMA | nat.BCAST_TRANSFER | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP

    def launch():
        nat.chain_device(stream=torch.cuda.current_stream().cuda_stream, n_waves=nw, n_points=N, n_steps=steps,
                         seg_len=lens, save_every=se, d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(),
                         d_alpha=d_a.data_ptr(), d_a0_soa=d_a0.data_ptr(), d_transfer_soa=d_tr.data_ptr(), flags=flags,
                         d_a_end_soa=d_aend.data_ptr(), d_p_end=d_pe.data_ptr(), d_p_max=d_pm.data_ptr(),
                         d_first_bad=d_bad.data_ptr(), d_workspace=d_ws.data_ptr())

    def check(ref):
        torch.cuda.synchronize()
        a_end = np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128)
        assert np.array_equal(a_end, ref["a_end"])
        assert np.array_equal(d_pe.cpu().numpy(), ref["p_end"]) and np.array_equal(d_pm.cpu().numpy(), ref["p_max"])
        assert np.array_equal(d_bad.cpu().numpy(), ref["first_bad_step"])

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch()
    side.synchronize()
    check(host)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    dbeta2 = rng.uniform(-0.03, 0.03, (S, N))
    d_db.copy_(torch.tensor(dbeta2, **f64))
    for t in (d_aend, d_pe, d_pm):
        t.zero_()
    graph.replay()
    check(nat.chain_host(dbeta2, n_steps=steps, seg_len=lens, save_every=se, gamma=gamma, alpha=alpha, a0=a0,
                         transfers=tr))
