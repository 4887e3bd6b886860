"""The float32 single-pump sweep on the GPU (psa_rk4_single_pump_f32: two sweep points per lane, packed math) against the
float64 NumPy restatement tests/single_pump_np.py fed the float32-ROUNDED inputs (dbeta, gamma, alpha and a0 are rounded to
float32 / complex64 first and then widened, so input rounding is not counted), at the project's bar RTOL_F32 (1e-4 of the
point's largest wave) with the wave_err / power_err measures of tests/wave_family.py.

Shapes are the smallest that can go wrong: 203 points are one full packed wave (128 points), a partial one and an odd tail;
1 500 steps are no multiple of RESYNC = 16; 65 541 points are 513 packed waves, the first size that takes 256-thread
workgroups.  Every test prints its measured worst case; on one MI355X: parity a_end 3.4e-6, p_wave_end 2.5e-6, p_wave_max
9.5e-7; loop edges 1.0e-7; 65 541 points x 40 steps against the float64 kernel 1.4e-7; trajectory rows 1.5e-6; signal gain and
idler conversion 2.3e-6 relative, pump depletion 1.5e-7; the gain spectrum 8.9e-6 dB from the float64 driver's."""
import functools

import numpy as np
import pytest

import psa_amd._native as nat
import single_pump_np
from conftest import RTOL_F32
from psa_amd import config, dispersion, scan_mismtach, sweep
from single_pump_np import GAMMA, LENGTH
from test_gpu_single_pump import _inputs
from wave_family import KEYS, power_err, wave_err

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else (np.uint32 if a.dtype == np.float32 else a.dtype))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def rounded_inputs(N, seed, per_point, lossy):
    """_inputs of the float64 test, rounded to float32 / complex64: -> (the float32 arrays, the same values widened)."""
    dbeta, a0, gamma, alpha = _inputs(N, seed, per_point, lossy)
    lo = dict(dbeta=np.asarray(dbeta, np.float32), a0=np.asarray(a0, np.complex64),
              gamma=np.asarray(gamma, np.float32) if per_point else np.float32(gamma),
              alpha=np.asarray(alpha, np.float32) if per_point else np.float32(alpha))
    hi = dict(dbeta=lo["dbeta"].astype(np.float64), a0=lo["a0"].astype(np.complex128),
              gamma=lo["gamma"].astype(np.float64) if per_point else float(lo["gamma"]),
              alpha=lo["alpha"].astype(np.float64) if per_point else float(lo["alpha"]))
    return lo, hi


def run32(lo, **kw):
    return nat.single_pump_host(lo["dbeta"], gamma=lo["gamma"], alpha=lo["alpha"], a0=lo["a0"], dtype=np.float32, **kw)


def restate(hi, **kw):
    return single_pump_np.integrate(hi["a0"], hi["dbeta"], gamma=hi["gamma"], alpha=hi["alpha"], **kw)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_case(per_point, lossy):
    """Rounded inputs and the restatement's every-step rows, computed once per case; any save stride is read off the rows."""
    lo, hi = rounded_inputs(203, 10 + 2 * per_point + lossy, per_point, lossy)
    ref = restate(hi, z_max=LENGTH, n=1500, save_every=1, want_traj=True)
    assert (ref["first_bad_step"] == -1).all()
    return lo, ref["traj"]


@pytest.mark.parametrize("save_every", [1, 7, 10])
@pytest.mark.parametrize("lossy", [True, False], ids=["lossy", "lossless"])
@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
def test_parity(per_point, lossy, save_every):
    lo, rows = _parity_case(per_point, lossy)
    r = run32(lo, n_steps=1500, z_max=LENGTH, save_every=save_every)
    saved = rows[:, ::save_every]
    err_a = wave_err(r["a_end"], saved[:, -1])
    err_e = power_err(r["p_wave_end"], np.abs(saved[:, -1]) ** 2)
    err_m = power_err(r["p_wave_max"], np.max(np.abs(saved) ** 2, axis=1))
    print(f"per_point={per_point} lossy={lossy} save_every={save_every}: a_end {err_a:.2e} p_wave_end {err_e:.2e} "
          f"p_wave_max {err_m:.2e}")
    assert r["a_end"].dtype == np.complex64 and r["p_wave_end"].dtype == np.float32 and r["p_wave_max"].dtype == np.float32
    assert (r["first_bad_step"] == -1).all()
    assert err_a < RTOL_F32 and err_e < RTOL_F32 and err_m < RTOL_F32


@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
def test_the_lossless_promise_selects_no_other_arithmetic(per_point):
    """alpha = 0 per point (the host form sets no flag), the same with PSA_OPT_LOSSLESS, and a broadcast alpha of 0 (the host
    form sets the flag itself): equal bits."""
    lo, _ = _parity_case(per_point, False)
    kw = dict(n_steps=1500, z_max=LENGTH, save_every=7, want_traj=True)
    plain = run32(dict(lo, alpha=np.zeros(203, np.float32)), **kw)
    promised = run32(dict(lo, alpha=np.zeros(203, np.float32)), extra_flags=nat.OPT_LOSSLESS, **kw)
    bcast = run32(dict(lo, alpha=np.float32(0.0)), **kw)
    for key in KEYS + ("traj",):
        assert same_bits(plain[key], promised[key]) and same_bits(plain[key], bcast[key]), key


# ---- 2. loop edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("save_every", [1, 4, 10])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 5, 15, 16, 17, 33])
def test_loop_edges(n_steps, save_every):
    """One step, an odd count, the re-seed at 16, one before and one past it, two re-seeds and a step, n_steps < save_every (the
    only row is z = 0: the outputs are a0) and tails that only the check runs."""
    lo, hi = rounded_inputs(70, 77, True, True)
    z_max = 0.5 * n_steps
    r = run32(lo, n_steps=n_steps, z_max=z_max, save_every=save_every)
    assert (r["first_bad_step"] == -1).all()
    if n_steps < save_every:
        assert same_bits(r["a_end"], lo["a0"]) and same_bits(r["p_wave_end"], r["p_wave_max"])
        assert np.max(np.abs(r["p_wave_end"].astype(np.float64) / np.abs(hi["a0"]) ** 2 - 1.0)) < 2.0 ** -22
        return
    ref = restate(hi, z_max=z_max, n=n_steps, save_every=save_every)
    err_a, err_e, err_m = (wave_err(r["a_end"], ref["a_end"]), power_err(r["p_wave_end"], ref["p_wave_end"]),
                           power_err(r["p_wave_max"], ref["p_wave_max"]))
    print(f"n_steps={n_steps} save_every={save_every}: {err_a:.2e} {err_e:.2e} {err_m:.2e}")
    assert err_a < RTOL_F32 and err_e < RTOL_F32 and err_m < RTOL_F32


# ---- 3. packing edges ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool():
    """203 points and their outputs in one launch: 50 steps cross three re-seeds, save_every 7 leaves a tail, with rows."""
    lo, _ = rounded_inputs(203, 41, True, True)
    kw = dict(n_steps=50, z_max=25.0, save_every=7, want_traj=True)
    return lo, kw, run32(lo, **kw)


@pytest.mark.parametrize("N", [1, 2, 3, 127, 128, 129, 203])
def test_a_point_does_not_depend_on_how_it_is_packed(N):
    """The first N points of one pool: a point's outputs are the same bits whichever N it ran in, and with the order of the
    points reversed -- which swaps the slots, changes the lane partners and (203 -> 128 + 75) moves points between the
    full-wave and the element-wise path.  No half reads its partner."""
    lo, kw, full = _pool()
    part = {k: v[:N] for k, v in lo.items()}
    fwd = run32(part, **kw)
    rev = run32({k: v[::-1].copy() for k, v in part.items()}, **kw)
    assert (full["first_bad_step"] == -1).all()
    for key in KEYS + ("traj",):
        assert same_bits(fwd[key], full[key][:N]), key
        assert same_bits(np.ascontiguousarray(rev[key][::-1]), full[key][:N]), key


# ---- 4. both workgroup sizes -----------------------------------------------------------------------------------------------
def test_both_block_sizes_agree_bit_for_bit():
    """65 541 points are 32 771 lanes = 513 packed waves: more than half the SIMDs, so the launch takes 256-thread workgroups,
    and the last lane holds the odd tail; PSA_OPT_BLOCK64 forces single-wave workgroups on the same points."""
    lo, hi = rounded_inputs(65541, 5, True, True)
    kw = dict(n_steps=40, z_max=20.0, save_every=10)
    big = run32(lo, **kw)
    small = run32(lo, extra_flags=nat.OPT_BLOCK64, **kw)
    for key in KEYS:
        assert same_bits(big[key], small[key]), key
    ref = nat.single_pump_host(hi["dbeta"], gamma=hi["gamma"], alpha=hi["alpha"], a0=hi["a0"], **kw)
    err_a, err_e, err_m = (wave_err(big["a_end"], ref["a_end"]), power_err(big["p_wave_end"], ref["p_wave_end"]),
                           power_err(big["p_wave_max"], ref["p_wave_max"]))
    print(f"65 541 points against the float64 kernel: a_end {err_a:.2e} p_wave_end {err_e:.2e} p_wave_max {err_m:.2e}")
    assert err_a < RTOL_F32 and err_e < RTOL_F32 and err_m < RTOL_F32
    assert (big["first_bad_step"] == -1).all() and (ref["first_bad_step"] == -1).all()


# ---- 5. failure index ------------------------------------------------------------------------------------------------------
HOT = (10, 21, 40, 41, 150, 153, 202)   # slot 0 beside a healthy slot 1, the reverse, both slots; the same in the partial wave; the odd tail


def test_failure_index_exact_block_and_unchecked():
    """gamma = 300 at the HOT points: gamma P h = 15, the explicit step is unstable and overflows within a few steps."""
    N, n, se = 203, 45, 10
    lo, hi = rounded_inputs(N, 3, True, True)
    hot = np.zeros(N, bool)
    hot[list(HOT)] = True
    sick = dict(lo, gamma=np.where(hot, np.float32(300.0), lo["gamma"]))
    kw = dict(n_steps=n, z_max=4.5, save_every=se)
    exact = run32(sick, exact_step=True, **kw)
    every = run32(sick, exact_step=True, n_steps=n, z_max=4.5, save_every=1, want_traj=True)
    finite_rows = np.isfinite(every["traj"].view(np.float32).reshape(N, n + 1, 6)).all(axis=2)
    first_row = np.where(finite_rows.all(axis=1), 0, np.argmin(finite_rows, axis=1))
    print("exact", exact["first_bad_step"][hot], "first non-finite row", first_row[hot])
    assert np.array_equal(exact["first_bad_step"], first_row - 1)
    assert np.array_equal(exact["first_bad_step"] >= 0, hot) and np.array_equal(every["first_bad_step"], exact["first_bad_step"])
    # the float64 restatement fails at exactly these points (its index may differ: float32 overflows earlier)
    ref = restate(dict(hi, gamma=np.where(hot, 300.0, hi["gamma"])), z_max=4.5, n=n, save_every=se)
    print("restatement", ref["first_bad_step"][hot])
    assert np.array_equal(ref["first_bad_step"] >= 0, hot)
    block = run32(sick, exact_step=False, **kw)
    b, e = block["first_bad_step"], exact["first_bad_step"]
    print("block", b[hot])
    assert np.array_equal(b == -1, e == -1)
    assert (b[hot] >= e[hot]).all() and (b[hot] < n).all() and (((b[hot] + 1) % se == 0) | (b[hot] == n - 1)).all()
    off = run32(sick, check_nan=False, **kw)
    assert (off["first_bad_step"] == -1).all()
    healthy = run32(lo, exact_step=True, **kw)
    assert (healthy["first_bad_step"] == -1).all()
    for r in (exact, block, off):
        for key in ("a_end", "p_wave_end", "p_wave_max"):
            assert same_bits(r[key][~hot], healthy[key][~hot]), key
        assert np.isnan(r["p_wave_max"][hot]).all()


# ---- 6. trajectory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("save_every", [1, 7])
def test_trajectory_rows(save_every):
    lo, rows = _parity_case(True, True)
    r = run32(lo, n_steps=1500, z_max=LENGTH, save_every=save_every, want_traj=True)
    saved = rows[:, ::save_every]
    assert r["traj"].shape == saved.shape and r["traj"].dtype == np.complex64 and same_bits(r["traj"][:, 0], lo["a0"])
    err = wave_err(r["traj"], saved)
    print(f"save_every={save_every}: rows {err:.2e}")
    assert err < RTOL_F32
    assert same_bits(r["traj"][:, -1], r["a_end"])
    dense = run32(lo, n_steps=1500, z_max=LENGTH, save_every=save_every)
    for key in KEYS:                                                        # the trajectory does not change the summary
        assert same_bits(dense[key], r[key]), key


def _device_run(torch, lo, *, n_steps, z_max, save_every, flags, traj_ld):
    """psa_rk4_single_pump_f32_dev on torch buffers -> the host entry's dictionary (traj from a [rows][3][ld][2] buffer)."""
    dev = torch.device("cuda:0")
    N = lo["dbeta"].size
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_db, d_g, d_al = t(lo["dbeta"]), t(np.atleast_1d(lo["gamma"])), t(np.atleast_1d(lo["alpha"]))
    d_a0 = t(lo["a0"].view(np.float32).reshape(N, 6).T)
    d_aend = torch.empty((6, N), dtype=torch.float32, device=dev)
    d_we, d_wm = torch.empty((3, N), dtype=torch.float32, device=dev), torch.empty((3, N), dtype=torch.float32, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    rows = n_steps // save_every + 1
    d_traj = torch.full((rows, 3, traj_ld, 2), -7.0, dtype=torch.float32, device=dev)
    nat.single_pump_device(stream=torch.cuda.current_stream().cuda_stream, n_points=N, n_steps=n_steps, z_max=z_max,
                           save_every=save_every, d_dbeta=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                           d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                           d_p_wave_end_soa=d_we.data_ptr(), d_p_wave_max_soa=d_wm.data_ptr(), d_first_bad=d_bad.data_ptr(),
                           d_traj_soa=d_traj.data_ptr(), dtype=np.float32)
    torch.cuda.synchronize()
    full = d_traj.cpu().numpy()                                              # [rows][3][ld][2]
    return dict(a_end=np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex64), p_wave_end=d_we.cpu().numpy().T,
                p_wave_max=d_wm.cpu().numpy().T, first_bad_step=d_bad.cpu().numpy(),
                traj=np.ascontiguousarray(full[:, :, :N].transpose(2, 0, 1, 3)).view(np.complex64)[..., 0], pad=full[:, :, N:])


@pytest.mark.parametrize("N,n_steps,save_every", [(300, 50, 7), (262144, 8, 4)], ids=["300", "262144"])
def test_device_entry_with_the_padded_leading_dimension(N, n_steps, save_every):
    """PSA_OPT_TRAJ_LD on the `_dev` form: 300 points keep ld = N; 262 144 points put the wave regions of a row 2 MiB apart and
    psa_traj_ld(N, 4) pads them by 544 points.  Equal to the host form (which pads internally) bit for bit; the padding
    columns are never written."""
    torch = pytest.importorskip("torch")
    ld = nat.traj_ld(N, np.float32)
    assert ld == (N if N == 300 else N + 544)
    lo, _ = rounded_inputs(N, 13, True, True)
    kw = dict(n_steps=n_steps, z_max=0.5 * n_steps, save_every=save_every)
    host = run32(lo, want_traj=True, **kw)
    got = _device_run(torch, lo, flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_TRAJ_LD, traj_ld=ld, **kw)
    for key in KEYS + ("traj",):
        assert same_bits(np.ascontiguousarray(got[key]), np.ascontiguousarray(host[key])), key
    assert got["traj"].shape == (N, n_steps // save_every + 1, 3) and got["pad"].shape[2] == ld - N and np.all(got["pad"] == -7.0)
    assert (host["first_bad_step"] == -1).all()


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------
def test_sweep_dtype_devices_and_reductions():
    """The reductions against the float64 call on the same (rounded) inputs.  RTOL_F32 bounds an amplitude error relative to the
    point's largest wave; a power ratio doubles a relative amplitude error, so signal_gain and idler_conversion (linear) are
    asked for 2e-4 relative and pump_depletion, a difference of two power ratios of order one, for 2e-4 absolute -- the
    equivalent of 1e-4 on the amplitudes.  Seeds of 1e-3 and 1e-5 W under a 0.5 W pump over 300 m: gains of a few, pump
    depletion of a few per cent."""
    N = 203
    rng = np.random.default_rng(17)
    dbeta = (rng.uniform(-3.5, -0.5, N) * GAMMA * 0.5).astype(np.float32)
    a0 = (np.sqrt(np.array([0.5, 1e-3, 1e-5])) * np.exp(1j * np.array([0.3, -1.0, 2.0]))).astype(np.complex64)
    gamma, alpha = np.float32(GAMMA), np.float32(1.15e-4)
    kw = dict(z_max=300.0, n_steps=3000, save_every=10, want_traj=True)
    one = sweep.rk4_sweep_single_pump(dbeta, gamma=gamma, alpha=alpha, a0=a0, dtype=np.float32, **kw)
    assert one.a_end.dtype == np.complex64 and one.traj.dtype == np.complex64 and one.traj.shape == (N, 301, 3)
    assert one.p_wave_end.dtype == np.float32 and one.p_wave_max.dtype == np.float32 and one.first_bad_step.dtype == np.int64
    assert same_bits(one.p_wave_in, (np.abs(a0) ** 2)[None, :].astype(np.float32)) and (one.first_bad_step == -1).all()
    two = sweep.rk4_sweep_single_pump(dbeta, gamma=gamma, alpha=alpha, a0=a0, dtype=np.float32, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert same_bits(getattr(one, key), getattr(two, key)), key
    ref = sweep.rk4_sweep_single_pump(dbeta.astype(np.float64), gamma=float(gamma), alpha=float(alpha), a0=a0.astype(np.complex128),
                                      **kw)
    assert ref.a_end.dtype == np.complex128
    p_s = float(np.abs(a0[1].astype(np.complex128)) ** 2)
    for mode in ("end", "max"):
        g = np.max(np.abs(one.signal_gain(p_s, mode=mode, unit="linear") / ref.signal_gain(p_s, mode=mode, unit="linear") - 1.0))
        c = np.max(np.abs(one.idler_conversion(p_s, mode=mode, unit="linear") / ref.idler_conversion(p_s, mode=mode, unit="linear") - 1.0))
        print(f"mode={mode}: signal_gain {g:.2e} idler_conversion {c:.2e} (relative)")
        assert g < 2e-4 and c < 2e-4
    d = np.max(np.abs(one.pump_depletion() - ref.pump_depletion()))
    print(f"pump_depletion {d:.2e} (absolute); largest depletion {ref.pump_depletion().max():.3f}, largest gain "
          f"{ref.signal_gain(p_s, unit='linear').max():.2f}")
    assert d < 2e-4 and ref.signal_gain(p_s, unit="linear").max() > 3.0


def test_gain_spectrum_driver_in_float32(golden):
    """scan_single_pump_gain(dtype=float32): the peak at dbeta = -2 gamma P_p (the sweep's spacing there is 0.05 gamma P_p) and the
    spectrum within 1e-3 dB of the float64 driver's."""
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    cfg = config.custom_simulation_config(z_max=300.0, dz=0.1)
    kw = dict(cfg=cfg, lambda_pump_m=1550e-9, lambda_signal_m=np.linspace(1530e-9, 1549.5e-9, 128), p_pump=0.5, p_signal=1e-9,
              gamma=GAMMA, alpha=0.0, dispersion=d, gain_mode="end")
    lo = scan_mismtach.scan_single_pump_gain(dtype=np.float32, **kw)
    hi = scan_mismtach.scan_single_pump_gain(**kw)
    assert lo["result"].a_end.dtype == np.complex64 and np.array_equal(lo["dbeta"], hi["dbeta"]) and lo["dbeta"].dtype == np.float64
    assert (lo["first_bad_step"] == -1).all() and np.isfinite(lo["gain"]).all()
    peak = lo["dbeta"][np.nanargmax(lo["gain"])] / (GAMMA * 0.5)
    err = np.max(np.abs(lo["gain"] - hi["gain"]))
    print(f"peak at dbeta = {peak:.3f} gamma P; gain against the float64 driver {err:.2e} dB, idler "
          f"{np.max(np.abs(lo['idler'] - hi['idler'])):.2e} dB")
    assert abs(peak + 2.0) < 0.1
    assert err < 1e-3
