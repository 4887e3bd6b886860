"""Single-pump fibre chains without a GPU: the gauge on the NumPy restatement (tests/single_pump_chain_np.py) against a direct
integration of the accumulated-phase model and against the copier - PSA closed form; the argument rules of
rk4_chain_single_pump, single_pump_mid_stage, run_concatenated_single_pump_simulation and scan_single_pump_copier_psa_phase;
every argument code of psa_rk4_single_pump_chain_f64 / _dev (all before any device call); the binding against the header; the
workspace size; the device split of a chain's points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psa_amd._native as nat
import single_pump_chain_np as chain_np
from conftest import RTOL_F64
from psa_amd._partition import CHAIN_AXES
from psa_amd.config import custom_simulation_config
from psa_amd.phase_matching import PhaseMatchingConfig, PhaseMatchingMethod
from psa_amd.scan_mismtach import scan_single_pump_copier_psa_phase
from psa_amd.simulation import mid_stage, run_concatenated_single_pump_simulation, single_pump_mid_stage
from psa_amd.sweep import FibreSpan, SinglePumpChainResult, SinglePumpResult, rk4_chain, rk4_chain_single_pump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS = -2, -3, -4, -5, -6, -7, -9, -11
A0 = np.sqrt(np.array([0.5, 1e-5, 1e-6])).astype(complex)


# ---- the gauge on the restatement ---------------------------------------------------------------------------------------
def test_gauge_reproduces_the_accumulated_phase_model():
    """24 random points, 3 lossy spans of 600, 1000 and 400 steps with per-point dbeta, gamma and alpha and complex per-point
    transfers: the B-frame run, span by span, against the direct RK4 of the accumulated-phase model, at RTOL_F64 of the point's
    largest wave (measured 1.7e-15).  The same run without the boundary phase is off by order 1."""
    a0, spans, transfers = chain_np.lossy_case(24)
    want = chain_np.direct(a0, spans, transfers, 50)
    got = chain_np.chain(a0, spans, transfers, 50)
    assert got["rows"].shape == want.shape == (24, sum(n // 50 + 1 for _, n, *_ in spans), 3)
    scale = np.abs(want).reshape(24, -1).max(axis=1)[:, None, None]
    err = float(np.max(np.abs(got["rows"] - want) / scale))
    wrong = float(np.max(np.abs(chain_np.chain(a0, spans, transfers, 50, gauge=False)["rows"] - want) / scale))
    print(f"gauge against the direct model: {err:.2e} of the largest wave; without the boundary phase {wrong:.2e}")
    assert err < RTOL_F64
    assert wrong > 1e-3
    assert np.array_equal(got["a_end"], got["rows"][:, -1]) and (got["first_bad_step"] == -1).all()


@pytest.mark.parametrize("cuts", [2, 3, 7])
def test_identity_split_on_the_restatement_equals_the_unsplit_run(cuts):
    n, se, L = 1400, 10, 700.0
    rng = np.random.default_rng(3)
    db, a0 = rng.uniform(-4.5, 0.5, 5) * 0.0115 * 0.5, A0 * np.exp(1j * rng.uniform(-3, 3, (5, 3)))
    whole = chain_np.chain(a0, [(L, n, db, 0.0115, 1.15e-4)], [], se)["rows"]
    steps = np.full(cuts, (n // se // cuts) * se)
    steps[-1] = n - steps[:-1].sum()
    got = chain_np.chain(a0, [(L * s / n, int(s), db, 0.0115, 1.15e-4) for s in steps], [np.ones(3)] * (cuts - 1), se)["rows"]
    offs = np.concatenate([[0], np.cumsum(steps)[:-1]])
    idx = np.concatenate([o // se + np.arange(s // se + 1) for o, s in zip(offs, steps)])
    assert np.max(np.abs(got - whole[:, idx])) < RTOL_F64 * np.max(np.abs(whole))


def test_restatement_matches_the_copier_psa_closed_form():
    """The signal gain of the lossless copier - PSA pair over K = 16 pump phases is a pure second harmonic: bin 0 and
    2 |bin 2| against the closed form at 1e-6 (measured 3e-9: the restatement's neglected depletion), every other bin below
    1e-8 of bin 0."""
    c = chain_np.closed_form_case()
    K = c["phases"].size
    T = np.ones((K, 3), complex)
    T[:, 0] = np.exp(1j * c["phases"])
    spans = [(L, n, np.full(K, db), c["gamma"], 0.0) for (db, L), n in zip((c["copier"], c["psa"]), c["steps"])]
    r = chain_np.chain(c["a0"], spans, [T], 50)
    e0, e2, rest = chain_np.check_harmonics(r["p_wave_end"][:, 1] / c["p_seed"], c["a"], c["b"])
    print(f"closed form: bin 0 {e0:.2e}, bin 2 {e2:.2e}, the other bins {rest:.2e} of bin 0")
    assert e0 < 1e-6 and e2 < 1e-6 and rest < 1e-8


# ---- argument rules of the Python layers (all raise before any native call) -------------------------------------------
def test_rk4_chain_single_pump_rules():
    s = [FibreSpan(10.0, n_steps=100, gamma=0.01), FibreSpan(10.0, n_steps=100, gamma=0.01)]
    with pytest.raises(ValueError, match="multiple of save_every"):
        rk4_chain_single_pump(s, a0=A0, save_every=7)
    with pytest.raises(ValueError, match="save_every"):
        rk4_chain_single_pump(s, a0=A0, save_every=0)
    with pytest.raises(ValueError, match="non-empty"):
        rk4_chain_single_pump([], a0=A0)
    with pytest.raises(ValueError, match="non-empty"):
        rk4_chain_single_pump([(10.0, 100)], a0=A0)
    with pytest.raises(ValueError, match="transfers"):
        rk4_chain_single_pump(s, a0=A0, transfers=[np.ones(3), np.ones(3)])
    with pytest.raises(ValueError, match="transfer must have shape"):
        rk4_chain_single_pump(s, a0=A0, transfers=[np.ones(4)])
    for a0 in (np.ones(4), np.ones(6), np.ones((2, 2, 3))):
        with pytest.raises(ValueError, match="a0"):
            rk4_chain_single_pump(s, a0=a0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_single_pump([FibreSpan(10.0, n_steps=100, dbeta=np.zeros(3)), FibreSpan(10.0, n_steps=100, dbeta=np.zeros(4))],
                              a0=A0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_single_pump([FibreSpan(10.0, n_steps=100, dbeta=np.zeros(3))], a0=np.ones((4, 3)))
    with pytest.raises(ValueError, match="gamma"):
        rk4_chain_single_pump([FibreSpan(10.0, n_steps=100, dbeta=np.zeros(3), gamma=np.zeros((3, 1)))], a0=A0)
    with pytest.raises(ValueError, match="dbeta2"):
        rk4_chain_single_pump([FibreSpan(10.0, n_steps=100, dbeta2=0.1)], a0=A0)
    with pytest.raises(ValueError, match="devices"):
        rk4_chain_single_pump(s, a0=A0, devices=[])
    # the 4- and 6-wave chain keeps rejecting three waves, and mid_stage three entries
    with pytest.raises(ValueError, match="a0"):
        rk4_chain(s, a0=A0)
    with pytest.raises(ValueError):
        mid_stage((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))


def test_single_pump_mid_stage():
    t = single_pump_mid_stage((0.0, -10.0, 3.0), (0.0, np.pi / 2, 0.1))
    np.testing.assert_allclose(np.abs(t) ** 2, 10.0 ** (np.array([0.0, -10.0, 3.0]) / 10.0), rtol=1e-15)
    np.testing.assert_allclose(np.angle(t)[1:], [np.pi / 2, 0.1], rtol=1e-15)
    assert np.array_equal(single_pump_mid_stage(), np.ones(3)) and single_pump_mid_stage(np.zeros((7, 3)), 0.0).shape == (7, 3)
    for bad in (((0.0,) * 4, (0.0,) * 4), (0.0, 0.0), ((0.0, np.nan, 0.0), (0.0,) * 3), ((0.0,) * 3, (0.0, np.inf, 0.0))):
        with pytest.raises(ValueError):
            single_pump_mid_stage(*bad)


def _dispersion(golden):
    from psa_amd.dispersion import DispersionParams
    dv = golden("G11")["disp_m"]
    return DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])


def test_run_concatenated_single_pump_simulation_rules(golden):
    pm = PhaseMatchingConfig(method=PhaseMatchingMethod.PROVIDED, provided_delta_beta=0.0)
    w = 2.0 * np.pi * 299792458.0 / 1550e-9
    span = dict(cfg=custom_simulation_config(z_max=1.0, dz=1e-2), gamma=0.01, alpha=0.0, phase_matching_cfg=pm)
    ok = dict(omega_pump=w, omega_signal=1.01 * w, p_in=[0.5, 1e-5, 0.0])
    run = run_concatenated_single_pump_simulation
    with pytest.raises(ValueError, match="at least one span"):
        run([], **ok)
    with pytest.raises(ValueError, match="unknown keys|needs cfg"):
        run([dict(span, bogus=1)], **ok)
    with pytest.raises(ValueError, match="needs cfg"):
        run([dict(cfg=span["cfg"], gamma=0.01, phase_matching_cfg=pm)], **ok)
    with pytest.raises(ValueError, match="exactly one of"):
        run([dict(span, dispersion=_dispersion(golden))], **ok)
    with pytest.raises(ValueError, match="exactly one of"):
        run([dict(cfg=span["cfg"], gamma=0.01, alpha=0.0)], **ok)
    with pytest.raises(ValueError, match="PROVIDED"):
        run([dict(span, phase_matching_cfg=PhaseMatchingConfig())], **ok)
    with pytest.raises(ValueError, match="max_order"):
        run([dict(cfg=span["cfg"], gamma=0.01, alpha=0.0, dispersion=_dispersion(golden), max_order=-1)], **ok)
    with pytest.raises(TypeError):
        run([dict(cfg=span["cfg"], gamma=0.01, alpha=0.0, dispersion="smf28")], **ok)
    with pytest.raises(ValueError, match="share save_every"):
        run([span, dict(span, cfg=custom_simulation_config(z_max=1.0, dz=1e-2, save_every=5))], **ok)
    with pytest.raises(ValueError, match="transfers"):
        run([span, span], transfers=[np.ones(3)] * 2, **ok)
    with pytest.raises(ValueError, match="transfers"):
        run([span, span], transfers=[np.ones(4)], **ok)
    with pytest.raises(ValueError, match="length_unit"):
        run([span], length_unit="mi", **ok)
    with pytest.raises(ValueError, match="multiple of save_every"):
        run([dict(span, cfg=custom_simulation_config(z_max=1.03, dz=1e-2))], **ok)
    for bad in (dict(omega_signal=2.0 * w), dict(omega_pump=-w), dict(omega_signal=np.inf), dict(p_in=[0.5, 1e-5]),
                dict(p_in=[0.5, -1e-5, 0.0]), dict(phase_in=[0.0] * 4)):
        with pytest.raises(ValueError):
            run([span], **dict(ok, **bad))
    with pytest.raises(ValueError):
        run([dict(span, cfg=custom_simulation_config(z_max=-1.0, dz=1e-2))], **ok)


def test_scan_single_pump_copier_psa_phase_rules():
    cfg = custom_simulation_config(z_max=10.0, dz=0.1)
    kw = dict(psa_cfg=cfg, psa_delta_beta=0.0, gamma=0.01, alpha=0.0, p_in=[0.5, 1e-5, 0.0])
    scan = scan_single_pump_copier_psa_phase
    for wave in ("pumps", "idler", 3, -1, 1.0, True):
        with pytest.raises(ValueError, match="phase_wave"):
            scan(**kw, phase_wave=wave)
    for db in (np.zeros((2, 2)), [], np.nan):
        with pytest.raises(ValueError, match="psa_delta_beta"):
            scan(**dict(kw, psa_delta_beta=db))
    for ph in ([], np.zeros((2, 2)), [0.0, np.inf]):
        with pytest.raises(ValueError, match="phase must"):
            scan(**kw, phase=ph)
    with pytest.raises(ValueError, match="gain_mode"):
        scan(**kw, gain_mode="mean")
    with pytest.raises(ValueError, match="gain_unit"):
        scan(**kw, gain_unit="neper")
    for p in ([0.5, 0.5, 1e-5, 0.0], [0.5, -1e-5, 0.0], [0.5, np.nan, 0.0]):
        with pytest.raises(ValueError, match="p_in"):
            scan(**dict(kw, p_in=p))
    with pytest.raises(ValueError, match="signal seed"):
        scan(**dict(kw, p_in=[0.5, 0.0, 1e-5]))
    with pytest.raises(ValueError, match="phase_in"):
        scan(**kw, phase_in=[0.0] * 4)
    with pytest.raises(ValueError):
        scan(**kw, mid_gain_db=(0.0,) * 4)
    with pytest.raises(ValueError):
        scan(**kw, mid_phase=(0.0,) * 4)
    with pytest.raises(ValueError, match="share save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.0, dz=0.1, save_every=5))
    with pytest.raises(ValueError, match="multiple of save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.3, dz=0.1))
    with pytest.raises(ValueError, match="length_unit"):
        scan(**kw, length_unit="mi")


# ---- the C-ABI validates before touching a device -------------------------------------------------------------------
def _call(host, **over):
    """psa_rk4_single_pump_chain_f64 (host) or _dev with dummy pointers: every call here must end in validation."""
    buf = np.zeros(256)
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(n=8, S=2, steps=[10, 20], lens=[1.0, 2.0], se=5, flags=0, null=False, traj=False, ws=p)
    a.update(over)
    steps = None if a["steps"] is None else np.asarray(a["steps"], dtype=np.int64)
    lens = None if a["lens"] is None else np.asarray(a["lens"], dtype=np.float64)
    sp = None if steps is None else steps.ctypes.data_as(C.c_void_p)
    lp = None if lens is None else lens.ctypes.data_as(C.c_void_p)
    q, t = (None if a["null"] else p), (p if a["traj"] else None)
    L = nat.lib()
    if host:
        return L.psa_rk4_single_pump_chain_f64(0, a["n"], a["S"], sp, lp, a["se"], p, p, p, p, None, a["flags"], p, p, q, p, t, None)
    return L.psa_rk4_single_pump_chain_f64_dev(None, a["n"], a["S"], sp, lp, a["se"], q, p, p, p, None, a["flags"], p, p, p, p, t,
                                               a["ws"])


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(host):
    call = lambda **over: _call(host, **over)   # noqa: E731
    assert call(S=0) == E_NSTEPS and call(S=-1) == E_NSTEPS
    assert call(steps=None) == E_NULLPTR and call(lens=None) == E_NULLPTR
    assert call(n=-1) == E_NPOINTS
    assert call(n=nat.MAX_POINTS + 1) == E_TOO_LARGE
    assert call(steps=[0, 20]) == E_NSTEPS and call(steps=[10, 0]) == E_NSTEPS and call(steps=[10, 5 * 2**29]) == E_NSTEPS
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(lens=[bad, 2.0]) == E_ZMAX and call(lens=[1.0, bad]) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(steps=[10, 21]) == E_SAVE_EVERY and call(steps=[11, 20]) == E_SAVE_EVERY
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT, nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED,
                nat.OPT_LDS_STAGING, 1 << 19, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    # the order: the span count, the first span's grid, the flags, the pointers, then the later spans
    assert call(S=0, n=-1) == E_NSTEPS and call(n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NPOINTS
    assert call(flags=nat.OPT_ONE_LANE, null=True) == E_FLAGS and call(null=True, steps=[10, 21]) == E_NULLPTR
    # a trajectory: ld * 16 < 2^32; without one the same size passes on to the next rule
    assert call(n=2**28, traj=True) == E_TOO_LARGE
    assert call(n=2**28, null=True) == E_NULLPTR and call(n=2**28 - 1, traj=True, null=True) == E_NULLPTR
    assert len(nat.lib().psa_last_error()) > 0


def test_flags_and_workspace_of_the_two_forms():
    ok = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.BCAST_TRANSFER | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP \
        | nat.OPT_LOSSLESS | nat.OPT_BLOCK64
    # every accepted bit passes validation: the next rule (a NULL pointer) is the one that answers
    assert _call(False, flags=ok | nat.OPT_TRAJ_LD, null=True) == E_NULLPTR and _call(True, flags=ok, null=True) == E_NULLPTR
    # the padded leading dimension belongs to the device form
    assert _call(True, flags=nat.OPT_TRAJ_LD) == E_FLAGS and _call(True, flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    # more than one span needs the caller's workspace on the _dev form; one span needs none (it stops at the launch or, on
    # a box without a device, before it -- never at the workspace rule)
    assert _call(False, ws=None) == E_NULLPTR and b"d_workspace" in nat.lib().psa_last_error()
    assert _call(False, n=0, ws=None) == 0


def test_an_empty_chain_is_a_successful_no_op():
    assert _call(False, n=0) == 0 and _call(True, n=0) == 0
    L = nat.lib()
    steps, lens = np.array([10], dtype=np.int64), np.array([1.0])
    sp, lp = steps.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)
    assert L.psa_rk4_single_pump_chain_f64_dev(None, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0
    assert L.psa_rk4_single_pump_chain_f64(0, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0


def test_workspace_bytes():
    """Theta and first_bad (8 N each), the next a0 and the span's a_end (48 N each), the span's two per-wave summaries (24 N
    each), every slice rounded up to 256 B."""
    def want(n):
        al = lambda b: (b + 255) // 256 * 256   # noqa: E731
        return 2 * al(8 * n) + 2 * al(48 * n) + 2 * al(24 * n)
    for n in (0, 1, 5, 32, 300, 65536, 10**6 + 7):
        assert nat.single_pump_chain_workspace_bytes(n) == want(n), n
    assert nat.single_pump_chain_workspace_bytes(-1) == -1 and nat.lib().psa_rk4_single_pump_chain_workspace_bytes(-2**40) == -1


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def test_the_binding_equals_the_header():
    """The three prototypes of include/psa_rk4.h, argument by argument, against the ctypes table; no new PSA_E_* code."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    for name, ret in (("psa_rk4_single_pump_chain_f64", "int"), ("psa_rk4_single_pump_chain_f64_dev", "int"),
                      ("psa_rk4_single_pump_chain_workspace_bytes", "int64_t")):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            args.append(C.c_void_p if "*" in decl else _CTYPE[decl.replace("const ", "").split()[0]])
        res, want = nat._SIGS[name]
        assert res is _CTYPE[ret] and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+(-\d+)", src)]
    assert sorted(codes) == list(range(-13, 0))


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    for S in (1, 2):
        with pytest.raises(nat.PsaNativeError) as e:
            nat.single_pump_chain_host(np.zeros((S, 3)), n_steps=[1] * S, seg_len=[1.0] * S, save_every=1, gamma=[1.0] * S,
                                       alpha=[0.0] * S, a0=np.ones(3, complex))
        assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)


def test_native_wrapper_shape_rules():
    kw = dict(dbeta=np.zeros((2, 3)), n_steps=[1, 1], seg_len=[1.0, 1.0], save_every=1, gamma=[1.0, 1.0], alpha=[0.0, 0.0],
              a0=np.ones(3, complex))
    for bad in (dict(dbeta=np.zeros(3)), dict(n_steps=[1]), dict(seg_len=[1.0] * 3), dict(gamma=[1.0]), dict(alpha=np.zeros((2, 2))),
                dict(a0=np.ones(4, complex)), dict(a0=np.ones((2, 3), complex)), dict(transfers=np.ones((1, 4), complex)),
                dict(transfers=np.ones((2, 3, 3), complex))):
        with pytest.raises(ValueError):
            nat.single_pump_chain_host(**dict(kw, **bad))
    with pytest.raises(ValueError):
        nat.single_pump_chain_device(stream=0, n_points=1, n_steps=[1, 2], seg_len=[1.0], save_every=1, d_dbeta=0, d_gamma=0,
                                     d_alpha=0, d_a0_soa=0, d_transfer_soa=0, flags=0, d_a_end_soa=0, d_p_wave_end_soa=0,
                                     d_p_wave_max_soa=0, d_first_bad=0)


# ---- devices=[...] ------------------------------------------------------------------------------------------------------
def test_devices_list_splits_the_chain_points_over_threads(monkeypatch):
    """rk4_chain_single_pump(devices=[...]) without a GPU: a spy in place of the native call sees contiguous blocks (4, 4, 3
    of 11 points), every per-point argument cut on its axis of CHAIN_AXES, broadcast ones whole; the outputs come back
    concatenated in point order."""
    seen = []

    def spy(dbeta, *, device, n_steps, seg_len, gamma, alpha, a0, transfers, **kw):
        n = dbeta.shape[1]
        assert set(kw) == {"save_every", "check_nan", "exact_step", "want_traj"}
        seen.append((int(device), n, dbeta.shape, gamma.shape, alpha.shape, a0.shape, transfers.shape, n_steps.shape))
        return dict(a_end=np.asarray(a0, dtype=complex), p_wave_end=np.stack([dbeta[0], gamma[1], transfers[0, :, 2].real], axis=1),
                    p_wave_max=np.abs(transfers[0]), first_bad_step=np.full(n, -1, dtype=np.int64), traj=None,
                    elapsed_ms=float(device) + 1.0)

    monkeypatch.setattr(nat, "single_pump_chain_host", spy)
    rng = np.random.default_rng(4)
    N = 11
    db0, gam1 = np.linspace(-0.02, 0.02, N), rng.uniform(5e-3, 2e-2, N)
    a0 = np.sqrt(rng.uniform(1e-5, 0.5, (N, 3))).astype(complex)
    T = np.exp(1j * rng.uniform(-3, 3, (N, 3))) * rng.uniform(0.5, 1.5, (N, 3))
    spans = [FibreSpan(10.0, n_steps=100, dbeta=db0, gamma=0.01, alpha=1e-4),
             FibreSpan(20.0, n_steps=200, dbeta=0.001, gamma=gam1, alpha=2e-4),
             FibreSpan(5.0, n_steps=50, dbeta=-0.003, gamma=0.01, alpha=1e-4)]
    one = rk4_chain_single_pump(spans, a0=a0, transfers=[T, np.ones(3)], devices=[0])
    assert seen == [(0, N, (3, N), (3, N), (3,), (N, 3), (2, N, 3), (3,))]
    seen.clear()
    many = rk4_chain_single_pump(spans, a0=a0, transfers=[T, np.ones(3)], devices=[0, 1, 2])
    assert sorted(seen) == [(d, n, (3, n), (3, n), (3,), (n, 3), (2, n, 3), (3,)) for d, n in ((0, 4), (1, 4), (2, 3))]
    assert set(CHAIN_AXES) >= {"dbeta", "gamma", "alpha", "a0", "transfers"}
    assert np.array_equal(many.a_end, a0) and np.array_equal(many.p_wave_end, np.stack([db0, gam1, T[:, 2].real], axis=1))
    assert np.array_equal(many.p_wave_max, np.abs(T)) and many.traj is None and many.elapsed_ms == 3.0
    assert isinstance(many, SinglePumpChainResult) and isinstance(many, SinglePumpResult)
    assert many.n_steps == 350 and many.save_every == 10 and np.array_equal(many.p_wave_in, np.abs(a0) ** 2)
    assert np.array_equal(many.step_offsets, [0, 100, 300, 350]) and np.array_equal(many.row_offsets, [0, 11, 32, 38])
    np.testing.assert_allclose(many.z_out[[0, 10, 11, 31, 32, 37]], [0.0, 10.0, 10.0, 30.0, 30.0, 35.0], rtol=1e-15)
    for f in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step", "z_out", "row_offsets", "step_offsets"):
        assert np.array_equal(getattr(one, f), getattr(many, f)), f
    # the reductions of SinglePumpResult work on a chain's result
    assert many.signal_gain(1.0, mode="end", unit="linear").shape == (N,) and many.pump_depletion().shape == (N,)
