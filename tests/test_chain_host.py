"""Fibre chains without a GPU: the argument rules of FibreSpan / rk4_chain / run_concatenated_simulation / mid_stage, the
C-ABI's argument errors (validated before any device use), and the gauge itself on the CPU oracle -- a chain integrated
span by span in the B frame (B_sig = A_sig e^{i Theta_s}) with the boundary rule of psa_chain.hip reproduces a direct
integration of the accumulated-phase model Theta(z) = sum_k dbeta_k L_k + dbeta_s zeta, and one fibre cut into spans
reproduces the unsplit oracle run."""
import ctypes as C

import numpy as np
import pytest

import oracle
import psa_amd._native as nat
from psa_amd.config import custom_simulation_config
from psa_amd.phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
from psa_amd.simulation import mid_stage, run_concatenated_simulation
from psa_amd.sweep import FibreSpan, rk4_chain

A0 = np.sqrt(np.array([0.5, 0.5, 1e-5, 1e-6])).astype(complex)


# ---- argument rules (all raise before any native call) ---------------------------------------------------------------
def test_fibre_span_rules():
    assert FibreSpan(100.0, dz=0.1).n_steps == 1000
    assert FibreSpan(100.0, n_steps=40).n_steps == 40
    for kw in (dict(length=0.0, dz=0.1), dict(length=float("inf"), dz=0.1), dict(length=1.0),
               dict(length=1.0, dz=0.1, n_steps=10), dict(length=1.0, dz=-0.1), dict(length=1.0, dz=10.0)):
        with pytest.raises(ValueError):
            FibreSpan(**kw)


def test_rk4_chain_rules():
    s = [FibreSpan(10.0, n_steps=100, gamma=0.01), FibreSpan(10.0, n_steps=100, gamma=0.01)]
    with pytest.raises(ValueError, match="multiple of save_every"):
        rk4_chain(s, a0=A0, save_every=7)
    with pytest.raises(ValueError, match="save_every"):
        rk4_chain(s, a0=A0, save_every=0)
    with pytest.raises(ValueError, match="non-empty"):
        rk4_chain([], a0=A0)
    with pytest.raises(ValueError, match="transfers"):
        rk4_chain(s, a0=A0, transfers=[np.ones(4), np.ones(4)])
    with pytest.raises(ValueError, match="transfer must have shape"):
        rk4_chain(s, a0=A0, transfers=[np.ones(5)])
    with pytest.raises(ValueError, match="a0"):
        rk4_chain(s, a0=np.ones(5))
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain([FibreSpan(10.0, n_steps=100, dbeta=np.zeros(3)), FibreSpan(10.0, n_steps=100, dbeta=np.zeros(4))],
                  a0=A0)
    with pytest.raises(ValueError, match="dbeta2"):
        rk4_chain(s, a0=np.ones(6))                       # 6 waves need dbeta2 in every span
    with pytest.raises(ValueError, match="dbeta2"):
        rk4_chain([FibreSpan(10.0, n_steps=100, dbeta2=0.1)], a0=A0)


def test_devices_list_splits_the_chain_points_over_threads(monkeypatch):
    """rk4_chain(devices=[...]) without a GPU: a spy chain_host sees contiguous blocks (4, 4, 3 of 11 points), every
    per-point argument cut on its own axis, broadcast ones whole, and the concatenated outputs come back in point order."""
    seen = []

    def spy(dbeta, *, device, n_steps, seg_len, gamma, alpha, a0, transfers, **kw):
        n = dbeta.shape[1]
        seen.append((int(device), n, dbeta.shape, gamma.shape, alpha.shape, a0.shape, transfers.shape, n_steps.shape))
        return dict(a_end=np.asarray(a0, dtype=complex), p_end=dbeta[0].copy(), p_max=gamma[1].copy(),
                    first_bad_step=np.full(n, -1, dtype=np.int64), traj=None, elapsed_ms=float(device) + 1.0,
                    p_wave_end=transfers[0].real.copy(), p_wave_max=None)

    monkeypatch.setattr(nat, "chain_host", spy)
    rng = np.random.default_rng(4)
    N = 11
    db0, gam1 = np.linspace(-0.02, 0.02, N), rng.uniform(5e-3, 2e-2, N)
    a0 = np.sqrt(rng.uniform(1e-5, 0.5, (N, 4))).astype(complex)
    T = np.exp(1j * rng.uniform(-3, 3, (N, 4)))
    spans = [FibreSpan(10.0, n_steps=100, dbeta=db0, gamma=0.01, alpha=1e-4),
             FibreSpan(20.0, n_steps=200, dbeta=0.001, gamma=gam1, alpha=2e-4),
             FibreSpan(5.0, n_steps=50, dbeta=-0.003, gamma=0.01, alpha=1e-4)]
    one = rk4_chain(spans, a0=a0, transfers=[T, np.ones(4)], devices=[0])
    seen.clear()
    many = rk4_chain(spans, a0=a0, transfers=[T, np.ones(4)], devices=[0, 1, 2])
    assert sorted(seen) == [(d, n, (3, n), (3, n), (3,), (n, 4), (2, n, 4), (3,)) for d, n in ((0, 4), (1, 4), (2, 3))]
    assert np.array_equal(many.a_end, a0) and np.array_equal(many.p_end, db0) and np.array_equal(many.p_max, gam1)
    assert np.array_equal(many.p_wave_end, T.real) and many.p_wave_max is None and many.traj is None
    assert many.elapsed_ms == 3.0
    for f in ("a_end", "p_end", "p_max", "first_bad_step", "p_wave_end", "z_out", "row_offsets", "step_offsets"):
        assert np.array_equal(getattr(one, f), getattr(many, f)), f


def test_mid_stage():
    t = mid_stage((0.0, -10.0, 3.0, 0.0), (0.0, 0.0, np.pi / 2, 0.1))
    np.testing.assert_allclose(np.abs(t) ** 2, 10.0 ** (np.array([0.0, -10.0, 3.0, 0.0]) / 10.0), rtol=1e-15)
    np.testing.assert_allclose(np.angle(t)[2:], [np.pi / 2, 0.1], rtol=1e-15)
    assert mid_stage(np.zeros((7, 6)), 0.0).shape == (7, 6)
    with pytest.raises(ValueError):
        mid_stage((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        mid_stage((0.0, 0.0, np.nan, 0.0))


def test_run_concatenated_simulation_rules():
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0)
    om = np.full(4, 1.2e15)
    span = dict(cfg=custom_simulation_config(z_max=1.0, dz=1e-2), gamma=0.01, alpha=0.0, phase_matching_cfg=pm)
    with pytest.raises(ValueError):
        run_concatenated_simulation([], omega=om, p_in=[0.5, 0.5, 1e-5, 0.0])
    with pytest.raises(ValueError, match="unknown keys|needs cfg"):
        run_concatenated_simulation([dict(span, bogus=1)], omega=om, p_in=[0.5, 0.5, 1e-5, 0.0])
    with pytest.raises(ValueError, match="share save_every"):
        run_concatenated_simulation([span, dict(span, cfg=custom_simulation_config(z_max=1.0, dz=1e-2, save_every=5))],
                                    omega=om, p_in=[0.5, 0.5, 1e-5, 0.0])
    with pytest.raises(ValueError, match="transfers"):
        run_concatenated_simulation([span, span], omega=om, p_in=[0.5, 0.5, 1e-5, 0.0], transfers=[np.ones(4)] * 2)
    with pytest.raises(ValueError, match="length_unit"):
        run_concatenated_simulation([span], omega=om, p_in=[0.5, 0.5, 1e-5, 0.0], length_unit="mi")


# ---- the C-ABI validates before touching a device -------------------------------------------------------------------
def _chain_dev(**over):
    buf = np.zeros(256)
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(n_waves=4, n_points=8, S=2, steps=[10, 20], lens=[1.0, 2.0], save_every=5, dbeta2=None, flags=0, traj=None,
             wend=None, wmax=None, ws=None)
    a.update(over)
    steps = np.asarray(a["steps"], dtype=np.int64)
    lens = np.asarray(a["lens"], dtype=np.float64)
    return nat.lib().psa_rk4_chain_f64_dev(None, a["n_waves"], a["n_points"], a["S"], steps.ctypes.data_as(C.c_void_p),
                                           lens.ctypes.data_as(C.c_void_p), a["save_every"], p, a["dbeta2"], p, p, p,
                                           None, a["flags"], p, p, p, p, a["traj"], a["wend"], a["wmax"], a["ws"])


@pytest.mark.parametrize("over,code", [
    (dict(n_waves=5), -1), (dict(n_points=-1), -2), (dict(S=0), -3), (dict(steps=[10, 0]), -3),
    (dict(lens=[1.0, 0.0]), -4), (dict(lens=[1.0, float("nan")]), -4), (dict(save_every=0), -5),
    (dict(steps=[10, 21]), -5), (dict(n_waves=6), -8), (dict(ws=None), -6),
    (dict(wend=C.c_void_p(8)), -6), (dict(wend=C.c_void_p(8), wmax=C.c_void_p(8), traj=C.c_void_p(8)), -11),
    (dict(flags=nat.OPT_SPLIT_POINT | nat.OPT_ONE_LANE), -11)])
def test_chain_argument_errors(over, code):
    assert _chain_dev(**over) == code
    assert len(nat.lib().psa_last_error()) > 0


def test_chain_null_arrays_and_workspace_size():
    L = nat.lib()
    assert L.psa_rk4_chain_f64_dev(None, 4, 8, 2, None, None, 5, *([None] * 6), 0, *([None] * 8)) == -6
    assert L.psa_rk4_chain_f64(0, 4, 8, 0, None, None, 5, *([None] * 6), 0, *([None] * 8)) == -3
    assert nat.chain_workspace_bytes(4, 1000) > 0 and nat.chain_workspace_bytes(6, 1000) > nat.chain_workspace_bytes(4, 1000)
    assert nat.chain_workspace_bytes(4, 1000, wave_summary=True) > nat.chain_workspace_bytes(4, 1000)
    assert L.psa_rk4_chain_workspace_bytes(5, 10, 8, 0) == -1 and L.psa_rk4_chain_workspace_bytes(4, 10, 2, 0) == -1
    # an empty chain is a valid no-op on the _dev face
    assert _chain_dev(n_points=0) == 0


# ---- the gauge on the CPU oracle --------------------------------------------------------------------------------------
def _oracle_chain(a0, spans, transfers, save_every):
    """Span by span through oracle.integrate (each span the reference model with its own dbeta and local z) in the B
    frame, boundary B' = T B with the signal times e^{i dbeta_s L_s}; rows brought back to A.  -> rows (A frame)."""
    theta, b, rows = 0.0, np.asarray(a0, dtype=complex), []
    for k, (L, n, db, g, al) in enumerate(spans):
        _, B, bad = oracle.integrate(b, z_max=L, n=n, save_every=save_every, gamma=g, alpha=al, dbeta=db)
        assert bad < 0
        A = B.copy()
        A[:, 2] *= np.exp(-1j * theta)
        rows.append(A)
        if k + 1 < len(spans):
            b = B[-1] * transfers[k]
            b[2] *= np.exp(1j * db * L)
            theta += db * L
    return np.concatenate(rows)


def _physical_chain(a0, spans, transfers, save_every):
    """Direct RK4 of the accumulated-phase model: the FWM factor e^{+-i Theta(z)} with Theta = Theta_s + dbeta_s zeta, in
    the A frame; the transfers applied to A.  (oracle.np_rhs with dbeta * z replaced by Theta.)"""
    theta0, y, rows = 0.0, np.asarray(a0, dtype=complex), []
    for k, (L, n, db, g, al) in enumerate(spans):
        # np_rhs(z, ...) forms dbeta * z: hand it z_eff = Theta / dbeta by giving dbeta = 1 and z = Theta
        def f(zeta, a):
            return oracle.np_rhs(theta0 + db * zeta, a, g, al, 1.0)
        zg = np.linspace(0.0, L, n + 1)
        out = [y.copy()]
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = f(z, y)
            k2 = f(z + 0.5 * h, y + 0.5 * h * k1)
            k3 = f(z + 0.5 * h, y + 0.5 * h * k2)
            k4 = f(z + h, y + h * k3)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            if (i + 1) % save_every == 0:
                out.append(y.copy())
        rows.append(np.array(out))
        if k + 1 < len(spans):
            y = y * transfers[k]
            theta0 += db * L
    return np.concatenate(rows)


def test_gauge_reproduces_the_accumulated_phase_model():
    spans = [(300.0, 600, 0.011, 0.0115, 1.2e-4), (200.0, 400, -0.007, 0.02, 0.0), (250.0, 500, 0.019, 0.009, 2e-4)]
    transfers = [mid_stage((-1.0, -2.0, 0.5, -3.0), (0.3, -0.2, 1.1, 0.0)), mid_stage((0.0, 0.0, 0.0, -1.0), (0.0, 2.0, 0.0, 0.4))]
    a0 = A0 * np.exp(1j * np.array([0.1, 0.4, -0.3, 0.2]))
    got = _oracle_chain(a0, spans, transfers, 50)
    want = _physical_chain(a0, spans, transfers, 50)
    assert got.shape == want.shape == (sum(n // 50 + 1 for _, n, *_ in spans), 4)
    scale = np.max(np.abs(want), axis=0)
    assert np.max(np.abs(got - want) / scale) < 1e-9
    # the gauge matters: without the boundary phase the signal is off by far more than rounding
    wrong = []
    theta, b = 0.0, a0.copy()
    for k, (L, n, db, g, al) in enumerate(spans):
        _, B, _ = oracle.integrate(b, z_max=L, n=n, save_every=50, gamma=g, alpha=al, dbeta=db)
        wrong.append(B)
        if k + 1 < len(spans):
            b = B[-1] * transfers[k]
    assert np.max(np.abs(np.concatenate(wrong) - want) / scale) > 1e-3


@pytest.mark.parametrize("cuts", [2, 3, 7])
def test_identity_split_on_the_oracle_equals_the_unsplit_run(cuts):
    n, se, L, db = 1400, 10, 700.0, 0.013
    _, whole, _ = oracle.integrate(A0, z_max=L, n=n, save_every=se, gamma=0.0115, alpha=1.15e-4, dbeta=db)
    steps = np.full(cuts, (n // se // cuts) * se)
    steps[-1] = n - steps[:-1].sum()
    spans = [(L * s / n, int(s), db, 0.0115, 1.15e-4) for s in steps]
    got = _oracle_chain(A0, spans, [np.ones(4)] * (cuts - 1), se)
    idx = np.concatenate([off // se + np.arange(s // se + 1) for off, s in zip(np.concatenate([[0], np.cumsum(steps)[:-1]]), steps)])
    assert np.max(np.abs(got - whole[idx]) / np.max(np.abs(whole), axis=0)) < 1e-9


# ---- the reference's chains (tests/golden/G17.npz, gen_golden_chain.py) on the CPU oracle -----------------------------
def _g17():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G17.npz"))


def _oracle_chain_rows(a0, spans, transfers, save_every):
    """spans: (length, dz, dbeta, gamma, alpha) rows -> A-frame rows of the whole chain (oracle.integrate + the gauge)."""
    rows = _oracle_chain(a0, [(L, int(round(L / dz)), db, g, al) for L, dz, db, g, al in spans], transfers, save_every)
    return rows


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("cuts", [1, 2, 3])
def test_oracle_chain_reproduces_g17_split(cuts):
    g = _g17()
    se, dz = int(g["save_every"]), float(g["split_dz"])
    steps = g[f"split{cuts}_steps"]
    for i, db in enumerate(g["split_dbeta"]):
        spans = [(s * dz, dz, db, float(g["split_gamma"]), float(g["split_alpha"])) for s in steps]
        rows = _oracle_chain_rows(np.sqrt(g["split_p_in"]).astype(complex), spans, [np.ones(4)] * (cuts - 1), se)
        assert _rel(rows, g[f"split{cuts}_A"][i]) < 1e-9
    # the reference itself: the split chains repeat the unsplit rows (to rounding) -- the gauge is right on its side too
    whole = g["split1_A"]
    idx = np.concatenate([o // se + np.arange(s // se + 1) for o, s in zip(np.concatenate([[0], np.cumsum(steps)[:-1]]), steps)])
    assert _rel(g[f"split{cuts}_A"], whole[:, idx]) < 1e-9


def test_oracle_chain_reproduces_g17_lossy():
    g = _g17()
    tr = [mid_stage(gd, ph) for gd, ph in zip(g["lossy_gain_db"], g["lossy_phase"])]
    for i, phi in enumerate(g["lossy_phase_in"]):
        a0 = np.sqrt(g["lossy_p_in"]).astype(complex)
        a0[2] *= np.exp(1j * phi)
        rows = _oracle_chain_rows(a0, g["lossy_spans"], tr, int(g["save_every"]))
        want = g["lossy_A"][i]
        assert np.max(np.abs(rows - want) / np.max(np.abs(want), axis=0)) < 1e-9


def test_oracle_chain_reproduces_g17_scan():
    g = _g17()
    L1, dz1, db1 = g["scan_copier"]
    L2, dz2 = g["scan_psa"]
    for k in (0, 7, 19, 31):
        for m, db2 in enumerate(g["scan_psa_dbeta"]):
            phi = g["scan_phases"][k]
            spans = [(L1, dz1, db1, float(g["scan_gamma"]), float(g["scan_alpha"])),
                     (L2, dz2, db2, float(g["scan_gamma"]), float(g["scan_alpha"]))]
            tr = [mid_stage(g["scan_mid_gain_db"], np.array([phi, phi, 0.0, 0.0]))]
            rows = _oracle_chain_rows(np.sqrt(g["scan_p_in"]).astype(complex), spans, tr, int(g["save_every"]))
            want = g["scan_A_end"][k, m]
            assert np.max(np.abs(rows[-1] - want) / np.abs(want).max()) < 1e-9
            assert abs(np.max(np.abs(rows[:, 2]) ** 2) / g["scan_p_sig_max"][k, m] - 1.0) < 1e-9


def test_scan_copier_psa_phase_rules():
    from psa_amd.scan_mismtach import scan_copier_psa_phase
    cfg = custom_simulation_config(z_max=10.0, dz=0.1)
    kw = dict(psa_cfg=cfg, psa_delta_beta=0.0, gamma=0.01, alpha=0.0, p_in=[0.5, 0.5, 1e-5, 0.0])
    with pytest.raises(ValueError, match="phase_wave"):
        scan_copier_psa_phase(**kw, phase_wave="idlers")
    with pytest.raises(ValueError, match="phase_wave"):
        scan_copier_psa_phase(**kw, phase_wave=4)
    with pytest.raises(ValueError, match="psa_delta_beta"):
        scan_copier_psa_phase(**dict(kw, psa_delta_beta=np.zeros((2, 2))))
    with pytest.raises(ValueError, match="phase must"):
        scan_copier_psa_phase(**kw, phase=[])
    with pytest.raises(ValueError, match="gain_mode"):
        scan_copier_psa_phase(**kw, gain_mode="mean")
    with pytest.raises(ValueError, match="share save_every"):
        scan_copier_psa_phase(**kw, copier_cfg=custom_simulation_config(z_max=10.0, dz=0.1, save_every=5))
    with pytest.raises(ValueError, match="multiple of save_every"):
        scan_copier_psa_phase(**kw, copier_cfg=custom_simulation_config(z_max=10.3, dz=0.1))
    with pytest.raises(ValueError, match="length_unit"):
        scan_copier_psa_phase(**kw, length_unit="mi")
