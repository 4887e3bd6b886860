"""Multi-channel fibre chains without a GPU: the K-signal gauge on the NumPy restatement (tests/pairs_chain_np.py) against a
direct integration of the accumulated-phase model and against the dual-pump copier - PSA closed form; the conditioning and
the failing case the GPU tests lean on; the argument rules of rk4_chain_pairs, rk4_sweep_pairs(want_traj), wdm_mid_stage and
scan_wdm_copier_psa_phase; every argument code of psa_rk4_pairs_chain_f64 / _dev (all before any device call); the binding
against the header; the workspace size; the device split of a chain's points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_chain_np as chain_np
import pairs_np
import psa_amd._native as nat
from conftest import RTOL_F64
from psa_amd._partition import PAIRS_CHAIN_AXES
from psa_amd.config import custom_simulation_config
from psa_amd.dispersion import DispersionParams, delta_beta_symmetric_array
from psa_amd.scan_mismtach import scan_wdm_copier_psa_phase
from psa_amd.simulation import mid_stage, wdm_mid_stage
from psa_amd.sweep import FibreSpan, PairsChainResult, PairsResult, rk4_chain, rk4_chain_pairs, rk4_sweep_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NPOINTS, E_NSTEPS, E_ZMAX, E_SAVE_EVERY, E_NULLPTR, E_DEVICE, E_TOO_LARGE, E_FLAGS, E_NPAIRS = -2, -3, -4, -5, -6, -7, -9, -11, -13
A0 = np.sqrt(np.array([0.25, 0.25, 1e-5, 1e-6, 2e-5, 0.0, 1e-6, 1e-6])).astype(complex)   # K = 3


def _scaled(got, want):
    n = want.shape[0]
    return float(np.max(np.abs(got - want) / np.abs(want).reshape(n, -1).max(axis=1).reshape((n,) + (1,) * (want.ndim - 1))))


# ---- the gauge on the restatement ---------------------------------------------------------------------------------------
def test_gauge_reproduces_the_accumulated_phase_model():
    """8 random points, K = 3, 3 lossy spans of 600, 1000 and 400 steps with per-point dbeta (N, K), gamma and alpha and complex
    transfers on every wave: the B-frame run, span by span, against the direct RK4 of the accumulated-phase model at 1e-12 of
    the point's largest wave (measured 1.4e-15).  dbeta L runs to +-4 rad per span, so the same run without the boundary phase
    is off by order 1 (measured 0.44)."""
    a0, spans, transfers = chain_np.lossy_case(8, 3)
    want = chain_np.direct(a0, spans, transfers, 50)
    got = chain_np.chain(a0, spans, transfers, 50)
    assert got["rows"].shape == want.shape == (8, sum(n // 50 + 1 for _, n, *_ in spans), 8)
    err = _scaled(got["rows"], want)
    wrong = _scaled(chain_np.chain(a0, spans, transfers, 50, gauge=False)["rows"], want)
    print(f"gauge against the direct model: {err:.2e} of the largest wave; without the boundary phase {wrong:.2e}")
    assert err < 1e-12
    assert wrong > 1e-3
    assert np.array_equal(got["a_end"], got["rows"][:, -1]) and (got["first_bad_step"] == -1).all()


def test_integrate_with_rows_is_pairs_np_integrate():
    rng = np.random.default_rng(7)
    a0, db = chain_np.random_a0(rng, 6, 3), rng.uniform(-0.02, 0.01, (6, 3))
    kw = dict(z_max=40.0, n=130, save_every=7, gamma=0.0115, alpha=1e-4)
    ref, got = pairs_np.integrate(a0, db, **kw), chain_np.integrate(a0, db, **kw)
    for key in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step"):
        assert np.array_equal(got[key], ref[key]), key
    assert got["traj"].shape == (6, 130 // 7 + 1, 8) and np.array_equal(got["traj"][:, 0], a0)


def test_the_cases_of_the_kernel_comparisons_are_well_conditioned():
    """test_gpu_pairs_chain compares K = 1 and K = 2 chains with rk4_chain's kernels, which order the triple products
    differently, at 1e-10.  That bar needs inputs whose rounding differences are not amplified: a relative input perturbation
    of 1e-14 on every amplitude moves the restatement's rows by less than 1e-12 (an amplification below 100)."""
    for K in (1, 2):
        a0, spans, transfers = chain_np.lossy_case(70, K, seed=21, steps=(60, 100, 40))
        rng = np.random.default_rng(3)
        base = chain_np.chain(a0, spans, transfers, 20)["rows"]
        moved = chain_np.chain(a0 * (1.0 + 1e-14 * rng.standard_normal(a0.shape)), spans, transfers, 20)["rows"]
        amp = _scaled(moved, base)
        print(f"K = {K}: a 1e-14 input perturbation moves the rows by {amp:.2e}")
        assert amp < 1e-12


def test_the_failing_case_fails_in_span_two():
    """The case of the GPU failure test: gamma = 300 in span 2 at points 1 and 3 overflows at local step 1, span 1 is finite."""
    a0, spans = chain_np.failing_case()
    first = chain_np.chain(a0, spans[:1], [], 10)
    assert (first["first_bad_step"] == -1).all() and np.all(np.isfinite(first["rows"]))
    ref = chain_np.chain(a0, spans, [np.ones(8)], 10)
    assert np.array_equal(ref["first_bad_step"], [-1, 401, -1, 401, -1])


def test_restatement_matches_the_dual_pump_closed_form():
    """The gain of every channel of the lossless WDM copier - PSA link over F = 16 pump phases is a pure second harmonic: bin 0
    and 2 |bin 2| against the closed form within a tenth of the GPU test's bar (measured <= 7.06e-9: the restatement's step
    error and neglected depletion), every other bin within a tenth of BAR_REST (measured <= 5.9e-11 of bin 0)."""
    c = chain_np.wdm_case()
    disp = DispersionParams(**c["disp"])
    wd = np.pi * 299792458.0 * (1.0 / c["lambda_p1_m"] - 1.0 / c["lambda_p2_m"])
    db = delta_beta_symmetric_array(wd, c["Omega"], disp, even_orders=(2, 4))
    x = db / (c["gamma"] * 2 * c["p_pump"])
    assert np.all((x > -2.7) & (x < -0.1)), x
    a, b = chain_np.closed_form_gain(db, c["lengths"][0], db, c["lengths"][1], c["gamma"], c["p_pump"], c["p_pump"])
    F, K = c["phases"].size, 4
    T = np.ones((F, 10), complex)
    T[:, :2] = np.exp(1j * c["phases"])[:, None]
    a_in = np.sqrt(np.array([c["p_pump"]] * 2 + [c["p_seed"], 0.0] * K)).astype(complex)
    r = chain_np.chain(a_in, [(L, n, db, c["gamma"], 0.0) for L, n in zip(c["lengths"], c["steps"])], [T], 50)
    for k in range(K):
        e0, e2, rest = chain_np.check_harmonics(r["p_wave_end"][:, 2 + 2 * k] / c["p_seed"], a[k], b[k])
        print(f"channel {k}: gain {a[k]:.3f} +- {b[k]:.3f}; bin 0 {e0:.2e}, bin 2 {e2:.2e}, the other bins {rest:.2e} of bin 0")
        assert 10.0 * max(e0, e2) <= c["BAR_BIN"] <= 1e-6 and 10.0 * rest <= c["BAR_REST"]


# ---- argument rules of the Python layers (all raise before any native call) -------------------------------------------
def test_rk4_chain_pairs_rules():
    def s(**kw):
        return [FibreSpan(10.0, n_steps=100, gamma=0.01, **dict(dict(dbeta=np.zeros(3)), **kw)) for _ in range(2)]
    with pytest.raises(ValueError, match="multiple of save_every"):
        rk4_chain_pairs(s(), a0=A0, save_every=7)
    with pytest.raises(ValueError, match="non-empty"):
        rk4_chain_pairs([], a0=A0)
    with pytest.raises(ValueError, match="dbeta2"):
        rk4_chain_pairs(s(dbeta2=np.zeros(3)), a0=A0)
    with pytest.raises(ValueError, match="transfers"):
        rk4_chain_pairs(s(), a0=A0, transfers=[np.ones(8), np.ones(8)])
    for width in (4, 6, 10, 7):
        with pytest.raises(ValueError, match="transfer must have shape"):
            rk4_chain_pairs(s(), a0=A0, transfers=[np.ones(width)])
    # dbeta: (K,) for every point or (N, K); K comes from a0
    for bad in (0.0, np.zeros(2), np.zeros(4), np.zeros((5, 2)), np.zeros((3, 5)), np.zeros((2, 5, 3))):
        with pytest.raises(ValueError, match="dbeta must have shape"):
            rk4_chain_pairs(s(dbeta=bad), a0=A0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_pairs([FibreSpan(10.0, n_steps=100, dbeta=np.zeros((5, 3))), FibreSpan(10.0, n_steps=100, dbeta=np.zeros((4, 3)))],
                        a0=A0)
    with pytest.raises(ValueError, match="disagree"):
        rk4_chain_pairs(s(dbeta=np.zeros((5, 3))), a0=np.ones((4, 8)))
    with pytest.raises(ValueError, match="dbeta must have shape"):
        rk4_chain_pairs(s(dbeta=np.zeros((1, 3)), alpha=np.zeros(5)), a0=A0)
    for a0 in (np.ones(3), np.ones(5), np.ones(36), np.ones(2), np.ones((2, 2, 8))):
        with pytest.raises(ValueError, match="a0"):
            rk4_chain_pairs(s(), a0=a0)
    with pytest.raises(ValueError, match="devices"):
        rk4_chain_pairs(s(), a0=A0, devices=[])
    # the 4- and 6-wave chain keeps its own rules: a (K,) dbeta there is N points
    with pytest.raises(ValueError, match="a0"):
        rk4_chain(s(), a0=A0)


def test_wdm_mid_stage():
    g = np.linspace(-3.0, 2.0, 8)
    t = wdm_mid_stage(g, np.linspace(-1.0, 1.0, 8))
    np.testing.assert_allclose(np.abs(t) ** 2, 10.0 ** (g / 10.0), rtol=1e-15)
    np.testing.assert_allclose(np.angle(t), np.linspace(-1.0, 1.0, 8), rtol=1e-15)
    for nw in range(4, 36, 2):
        assert wdm_mid_stage(np.zeros((7, nw)), 0.0).shape == (7, nw)
    assert np.array_equal(wdm_mid_stage(np.zeros(4), np.zeros(4)), mid_stage())
    for bad in ((np.zeros(3), 0.0), (np.zeros(5), 0.0), (np.zeros(36), 0.0), (0.0, 0.0), (np.full(8, np.nan), 0.0), (np.zeros(8), np.inf)):
        with pytest.raises(ValueError):
            wdm_mid_stage(*bad)


def test_scan_wdm_copier_psa_phase_rules():
    c = chain_np.wdm_case()
    cfg = custom_simulation_config(z_max=10.0, dz=0.1)
    kw = dict(psa_cfg=cfg, lambda_p1_m=c["lambda_p1_m"], lambda_p2_m=c["lambda_p2_m"], Omega=c["Omega"], p_pump=[0.25, 0.25],
              p_signal=[1e-6] * 4, gamma=0.0115, alpha=0.0, dispersion=DispersionParams(**c["disp"]))
    scan = scan_wdm_copier_psa_phase
    for wave in ("pump", "signal", 0, None):
        with pytest.raises(ValueError, match="phase_wave"):
            scan(**kw, phase_wave=wave)
    for ph in ([], np.zeros((2, 2)), [0.0, np.inf]):
        with pytest.raises(ValueError, match="phase must"):
            scan(**kw, phase=ph)
    with pytest.raises(ValueError, match="gain_mode"):
        scan(**kw, gain_mode="mean")
    with pytest.raises(ValueError, match="gain_unit"):
        scan(**kw, gain_unit="neper")
    for bad in (dict(Omega=[]), dict(Omega=np.ones(17)), dict(Omega=[1.0, np.nan, 1.0, 1.0]), dict(Omega=[1e20] * 4),
                dict(p_pump=[0.5]), dict(p_pump=[0.5, -0.1]), dict(p_signal=[1e-6] * 3), dict(p_signal=[1e-6, 0.0, 1e-6, 1e-6]),
                dict(p_signal=np.full((2, 4), 1e-6)), dict(p_idler=[0.0] * 3), dict(p_idler=-1.0), dict(mid_gain_db=np.zeros(4)),
                dict(mid_phase=np.zeros(8)), dict(dispersion=None)):
        with pytest.raises(ValueError):
            scan(**dict(kw, **bad))
    with pytest.raises(ValueError, match="share save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.0, dz=0.1, save_every=5))
    with pytest.raises(ValueError, match="multiple of save_every"):
        scan(**kw, copier_cfg=custom_simulation_config(z_max=10.3, dz=0.1))
    with pytest.raises(ValueError, match="length_unit"):
        scan(**kw, length_unit="mi")


# ---- the C-ABI validates before touching a device -------------------------------------------------------------------
def _call(host, **over):
    """psa_rk4_pairs_chain_f64 (host) or _dev with dummy pointers: every call here must end in validation."""
    buf = np.zeros(256)
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(K=3, n=8, S=2, steps=[10, 20], lens=[1.0, 2.0], se=5, flags=0, null=False, traj=False, ws=p)
    a.update(over)
    steps = None if a["steps"] is None else np.asarray(a["steps"], dtype=np.int64)
    lens = None if a["lens"] is None else np.asarray(a["lens"], dtype=np.float64)
    sp = None if steps is None else steps.ctypes.data_as(C.c_void_p)
    lp = None if lens is None else lens.ctypes.data_as(C.c_void_p)
    q, t = (None if a["null"] else p), (p if a["traj"] else None)
    L = nat.lib()
    if host:
        return L.psa_rk4_pairs_chain_f64(0, a["K"], a["n"], a["S"], sp, lp, a["se"], p, p, p, p, None, a["flags"], p, p, q, p, t, None)
    return L.psa_rk4_pairs_chain_f64_dev(None, a["K"], a["n"], a["S"], sp, lp, a["se"], q, p, p, p, None, a["flags"], p, p, p, p, t,
                                         a["ws"])


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
def test_every_argument_error_comes_back_before_any_device_call(host):
    call = lambda **over: _call(host, **over)   # noqa: E731
    assert call(S=0) == E_NSTEPS and call(S=-1) == E_NSTEPS
    assert call(steps=None) == E_NULLPTR and call(lens=None) == E_NULLPTR
    for K in (0, 17, -1):
        assert call(K=K) == E_NPAIRS
    assert call(n=-1) == E_NPOINTS
    # the launch grid: 2 * PSA_MAX_POINTS lanes, L lanes per point
    assert call(K=1, n=nat.MAX_POINTS + 1) == E_TOO_LARGE and call(K=16, n=2 * nat.MAX_POINTS // 16 + 1) == E_TOO_LARGE
    assert call(K=16, n=2 * nat.MAX_POINTS // 16, null=True) == E_NULLPTR
    assert call(steps=[0, 20]) == E_NSTEPS and call(steps=[10, 0]) == E_NSTEPS and call(steps=[10, 5 * 2**29]) == E_NSTEPS
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(lens=[bad, 2.0]) == E_ZMAX and call(lens=[1.0, bad]) == E_ZMAX
    assert call(se=0) == E_SAVE_EVERY
    assert call(steps=[10, 21]) == E_SAVE_EVERY and call(steps=[11, 20]) == E_SAVE_EVERY
    # one span alone is the sweep's trajectory form: it may end behind its last saved row, as the sweep may
    assert call(S=1, steps=[11], lens=[1.0], null=True) == E_NULLPTR and call(S=1, steps=[11], lens=[1.0], n=0) == 0
    assert call(S=1, steps=[11], lens=[1.0], traj=True, n=0) == 0
    assert call(null=True) == E_NULLPTR
    for bit in (nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT, nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED,
                nat.OPT_LDS_STAGING, 1 << 19, 1 << 30):
        assert call(flags=bit | nat.OPT_CHECK_NAN) == E_FLAGS, bit
    # the order: the span count, n_pairs, the first span's grid, the flags, the pointers, then the later spans
    assert call(S=0, K=0) == E_NSTEPS and call(K=0, n=-1) == E_NPAIRS and call(n=-1, flags=nat.OPT_ONE_LANE, null=True) == E_NPOINTS
    assert call(flags=nat.OPT_ONE_LANE, null=True) == E_FLAGS and call(null=True, steps=[10, 21]) == E_NULLPTR
    # a trajectory: ld * 16 < 2^32; without one the same size passes on to the next rule
    assert call(K=1, n=2**28, traj=True) == E_TOO_LARGE and call(K=3, n=2**28, traj=True) == E_TOO_LARGE
    assert call(K=1, n=2**28, null=True) == E_NULLPTR and call(K=1, n=2**28 - 1, traj=True, null=True) == E_NULLPTR
    assert len(nat.lib().psa_last_error()) > 0


def test_flags_and_workspace_of_the_two_forms():
    ok = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.BCAST_TRANSFER | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP \
        | nat.OPT_LOSSLESS | nat.OPT_BLOCK64
    # every accepted bit passes validation: the next rule (a NULL pointer) is the one that answers
    assert _call(False, flags=ok | nat.OPT_TRAJ_LD, null=True) == E_NULLPTR and _call(True, flags=ok, null=True) == E_NULLPTR
    # the padded leading dimension belongs to the chain's device form, not to its host form ...
    assert _call(True, flags=nat.OPT_TRAJ_LD) == E_FLAGS and _call(True, flags=nat.OPT_TRAJ_LD, traj=True) == E_FLAGS
    assert b"multi-channel chain" in nat.lib().psa_last_error()
    # ... nor to the sweep's entry points, which answer as they did
    p = np.zeros(64).ctypes.data_as(C.c_void_p)
    assert nat.lib().psa_rk4_sweep_pairs_f64_dev(None, 3, 8, 10, 1.0, 5, p, p, p, p, nat.OPT_TRAJ_LD, p, p, p, p) == E_FLAGS
    assert b"multi-channel sweep" in nat.lib().psa_last_error()
    # more than one span needs the caller's workspace on the _dev form
    assert _call(False, ws=None) == E_NULLPTR and b"d_workspace" in nat.lib().psa_last_error()
    assert _call(False, n=0, ws=None) == 0


def test_an_empty_chain_is_a_successful_no_op():
    assert _call(False, n=0) == 0 and _call(True, n=0) == 0
    L = nat.lib()
    steps, lens = np.array([10], dtype=np.int64), np.array([1.0])
    sp, lp = steps.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p)
    assert L.psa_rk4_pairs_chain_f64_dev(None, 3, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0
    assert L.psa_rk4_pairs_chain_f64(0, 3, 0, 1, sp, lp, 5, *([None] * 5), 0, *([None] * 6)) == 0


def test_workspace_bytes():
    """Theta [K][N] in one block and first_bad (8 N), the next a0 and the span's a_end (16 NW N each), the span's two per-wave
    summaries (8 NW N each), every slice rounded up to 256 B; -1 for a call no chain takes; monotone in K."""
    def want(k, n):
        al = lambda b: (b + 255) // 256 * 256   # noqa: E731
        nw = 2 + 2 * k
        return al(8 * k * n) + al(8 * n) + 2 * al(16 * nw * n) + 2 * al(8 * nw * n)
    for n in (0, 1, 5, 32, 300, 65536, 10**6 + 7):
        sizes = [nat.pairs_chain_workspace_bytes(k, n) for k in range(1, 17)]
        assert sizes == [want(k, n) for k in range(1, 17)], n
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and (n == 0 or sizes[-1] > sizes[0])
    for k, n in ((0, 8), (17, 8), (-1, 8), (3, -1), (3, -2**40)):
        assert nat.lib().psa_rk4_pairs_chain_workspace_bytes(k, n) == -1
    # the two sizes that were there stay what they were
    assert nat.chain_workspace_bytes(6, 300, np.float64, True) == 2 * 2560 + 2 * 28928 + 3 * 2560 + 2 * 14592
    assert nat.single_pump_chain_workspace_bytes(300) == 2 * 2560 + 2 * 14592 + 2 * 7424


_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double}


def test_the_binding_equals_the_header():
    """The three prototypes of include/psa_rk4.h, argument by argument, against the ctypes table; no new PSA_E_* code; the
    sweep's two prototypes are what they were."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "psa_rk4.h"), encoding="utf-8").read(), flags=re.S)
    for name, ret in (("psa_rk4_pairs_chain_f64", "int"), ("psa_rk4_pairs_chain_f64_dev", "int"),
                      ("psa_rk4_pairs_chain_workspace_bytes", "int64_t"), ("psa_rk4_sweep_pairs_f64", "int"),
                      ("psa_rk4_sweep_pairs_f64_dev", "int")):
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        args = []
        for decl in m.group(1).split(","):
            decl = decl.strip()
            args.append(C.c_void_p if "*" in decl else _CTYPE[decl.replace("const ", "").split()[0]])
        res, want = nat._SIGS[name]
        assert res is _CTYPE[ret] and list(want) == args, name
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), name)
    assert len(nat._SIGS["psa_rk4_pairs_chain_f64"][1]) == 19 and len(nat._SIGS["psa_rk4_sweep_pairs_f64"][1]) == 16
    codes = [int(x) for x in re.findall(r"#define\s+PSA_E_\w+\s+(-\d+)", src)]
    assert sorted(codes) == list(range(-13, 0))


@pytest.mark.skipif(nat.device_count() > 0, reason="CPU box only")
def test_without_a_device_a_valid_call_is_an_error_not_a_fallback():
    for S in (1, 2):
        with pytest.raises(nat.PsaNativeError) as e:
            nat.pairs_chain_host(np.zeros((S, 3, 2)), n_steps=[1] * S, seg_len=[1.0] * S, save_every=1, gamma=[1.0] * S,
                                 alpha=[0.0] * S, a0=np.ones(6, complex), want_traj=True)
        assert e.value.code == E_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(nat.PsaNativeError) as e:
        rk4_sweep_pairs(np.zeros((3, 2)), z_max=1.0, n_steps=4, save_every=2, gamma=1.0, alpha=0.0, a0=np.ones(6, complex),
                        want_traj=True)
    assert e.value.code == E_DEVICE


def test_native_wrapper_shape_rules():
    kw = dict(dbeta=np.zeros((2, 3, 2)), n_steps=[1, 1], seg_len=[1.0, 1.0], save_every=1, gamma=[1.0, 1.0], alpha=[0.0, 0.0],
              a0=np.ones(6, complex))
    for bad in (dict(dbeta=np.zeros((2, 3))), dict(dbeta=np.zeros((2, 3, 17))), dict(dbeta=np.zeros((2, 3, 0))), dict(n_steps=[1]),
                dict(seg_len=[1.0] * 3), dict(gamma=[1.0]), dict(alpha=np.zeros((2, 2))), dict(a0=np.ones(4, complex)),
                dict(a0=np.ones((2, 6), complex)), dict(transfers=np.ones((1, 4), complex)),
                dict(transfers=np.ones((2, 3, 6), complex))):
        with pytest.raises(ValueError):
            nat.pairs_chain_host(**dict(kw, **bad))
    with pytest.raises(ValueError):
        nat.pairs_chain_device(stream=0, n_pairs=2, n_points=1, n_steps=[1, 2], seg_len=[1.0], save_every=1, d_dbeta_soa=0,
                               d_gamma=0, d_alpha=0, d_a0_soa=0, d_transfer_soa=0, flags=0, d_a_end_soa=0, d_p_wave_end_soa=0,
                               d_p_wave_max_soa=0, d_first_bad=0)


# ---- devices=[...] ------------------------------------------------------------------------------------------------------
def test_devices_list_splits_the_chain_points_over_threads(monkeypatch):
    """rk4_chain_pairs(devices=[...]) and rk4_sweep_pairs(want_traj=True, devices=[...]) without a GPU: a spy in place of the
    native call sees contiguous blocks (4, 4, 3 of 11 points), every per-point argument cut on its axis of PAIRS_CHAIN_AXES,
    broadcast ones whole; the outputs come back concatenated in point order."""
    seen = []

    def spy(dbeta, *, device, n_steps, seg_len, gamma, alpha, a0, transfers=None, **kw):
        n, nw = dbeta.shape[1], 2 + 2 * dbeta.shape[2]
        assert set(kw) == {"save_every", "check_nan", "exact_step", "want_traj"}
        seen.append((int(device), n, dbeta.shape, np.shape(gamma), np.shape(alpha), a0.shape,
                     None if transfers is None else transfers.shape, np.shape(n_steps)))
        rows = int(np.sum(np.asarray(n_steps) // kw["save_every"] + 1))
        return dict(a_end=np.broadcast_to(np.asarray(a0, dtype=complex), (n, nw)).copy(), p_wave_end=np.tile(dbeta[0], (1, nw))[:, :nw],
                    p_wave_max=np.abs(np.broadcast_to(a0, (n, nw))) + 0.0, first_bad_step=np.full(n, -1, dtype=np.int64),
                    traj=np.zeros((n, rows, nw), complex) if kw["want_traj"] else None, elapsed_ms=float(device) + 1.0)

    monkeypatch.setattr(nat, "pairs_chain_host", spy)
    rng = np.random.default_rng(4)
    N, K = 11, 3
    db0, gam1 = rng.uniform(-0.02, 0.02, (N, K)), rng.uniform(5e-3, 2e-2, N)
    a0 = np.sqrt(rng.uniform(1e-5, 0.5, (N, 8))).astype(complex)
    T = np.exp(1j * rng.uniform(-3, 3, (N, 8))) * rng.uniform(0.5, 1.5, (N, 8))
    spans = [FibreSpan(10.0, n_steps=100, dbeta=db0, gamma=0.01, alpha=1e-4),
             FibreSpan(20.0, n_steps=200, dbeta=np.array([1e-3, 2e-3, 3e-3]), gamma=gam1, alpha=2e-4),
             FibreSpan(5.0, n_steps=50, dbeta=np.zeros(3), gamma=0.01, alpha=1e-4)]
    one = rk4_chain_pairs(spans, a0=a0, transfers=[T, np.ones(8)], devices=[0])
    assert seen == [(0, N, (3, N, K), (3, N), (3,), (N, 8), (2, N, 8), (3,))]
    seen.clear()
    many = rk4_chain_pairs(spans, a0=a0, transfers=[T, np.ones(8)], devices=[0, 1, 2])
    assert sorted(seen) == [(d, n, (3, n, K), (3, n), (3,), (n, 8), (2, n, 8), (3,)) for d, n in ((0, 4), (1, 4), (2, 3))]
    assert set(PAIRS_CHAIN_AXES) == {"dbeta", "gamma", "alpha", "a0", "transfers"} and PAIRS_CHAIN_AXES["dbeta"] == (1, 3)
    assert np.array_equal(many.a_end, a0) and many.traj is None and many.elapsed_ms == 3.0
    assert isinstance(many, PairsChainResult) and isinstance(many, PairsResult) and many.n_pairs == K
    assert many.n_steps == 350 and many.save_every == 10 and np.array_equal(many.p_wave_in, np.abs(a0) ** 2)
    assert np.array_equal(many.step_offsets, [0, 100, 300, 350]) and np.array_equal(many.row_offsets, [0, 11, 32, 38])
    np.testing.assert_allclose(many.z_out[[0, 10, 11, 31, 32, 37]], [0.0, 10.0, 10.0, 30.0, 30.0, 35.0], rtol=1e-15)
    for f in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step", "z_out", "row_offsets", "step_offsets"):
        assert np.array_equal(getattr(one, f), getattr(many, f)), f
    assert many.channel_gain(np.full(K, 1e-5), mode="end", unit="linear").shape == (N, K) and many.pump_depletion().shape == (N,)
    # the sweep's trajectory form is one span of the same entry point
    seen.clear()
    r = rk4_sweep_pairs(db0, z_max=10.0, n_steps=100, save_every=10, gamma=gam1, alpha=1e-4, a0=a0, want_traj=True, devices=[0, 1, 2])
    assert sorted(seen) == [(d, n, (1, n, K), (1, n), (1,), (n, 8), None, (1,)) for d, n in ((0, 4), (1, 4), (2, 3))]
    assert isinstance(r, PairsResult) and r.traj.shape == (N, 11, 8) and r.n_steps == 100
