"""The float32 multi-line ("frequency comb") sweep on the GPU (psa_rk4_comb_f32: two sweep points per lane, packed math) against
the NumPy restatement tests/comb_np.py in float64, fed the float32-rounded inputs the kernel sees, at the project's float32 bar
RTOL_F32 (1e-4 of the point's largest line): parity, the lossless promise, the loop's edges around the 16-step seed grid, the
packing (a point's result depends neither on N nor on its half), both block sizes, dark lines, the failure index per half, the
rows, the device entry and the two drivers.  Shapes are the smallest that can go wrong: 203 points are one full packed wave and
a ragged one with an odd tail, 1 500 steps are no multiple of the seed interval, M = 3 and 12 are the ends of the range, 4 the
smallest even comb, 7 the first that needs more than 256 registers, 12 the one that keeps three vectors in LDS."""
import functools

import numpy as np
import pytest

import comb_np
import psa_amd._native as nat
import wave_family
from conftest import RTOL_F32
from psa_amd import config, dispersion, scan_mismtach, sweep
from wave_family import KEYS

pytestmark = pytest.mark.gpu

F32, C64 = np.float32, np.complex64
Z_MAX, N_STEPS = 300.0, 1500
RESYNC = 16                      # psa_rk4_comb_pk_kernel.inc.h: COMB_PK_RESYNC, the seed interval shipped


def wave_err(got, ref):
    """wave_family.wave_err of the float32 outputs, widened first."""
    return wave_family.wave_err(np.asarray(got, dtype=np.complex128), ref)


def power_err(got, ref):
    """wave_family.power_err of the float32 outputs, widened first: the moduli are formed in float64."""
    return wave_family.power_err(np.asarray(got, dtype=np.float64), ref)


def rounded_inputs(*args, **kw):
    """comb_np.random_inputs as the float32 entry points see them: each value rounded once (float32 / complex64 arrays)."""
    kappa, a0, gamma, alpha = comb_np.random_inputs(*args, **kw)
    return kappa.astype(F32), np.asarray(a0).astype(C64), np.asarray(gamma, dtype=F32), np.asarray(alpha, dtype=F32)


def reference(kappa, a0, gamma, alpha, **kw):
    """The float64 restatement on the rounded values (their widening is exact)."""
    return comb_np.integrate(np.asarray(a0, dtype=np.complex128), np.asarray(kappa, dtype=np.float64),
                             gamma=np.asarray(gamma, dtype=np.float64), alpha=np.asarray(alpha, dtype=np.float64), **kw)


def run(kappa, **kw):
    return nat.comb_host(kappa, dtype=F32, **kw)


def same(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]).view(np.asarray(a[key]).real.dtype), np.asarray(b[key]).view(np.asarray(b[key]).real.dtype),
                              equal_nan=True), key


@functools.lru_cache(maxsize=None)
def _parity_case(M, per_point, lossy):
    """Inputs and the restatement's every-step rows, computed once per case; any save stride is read off the rows."""
    kappa, a0, gamma, alpha = rounded_inputs(203, M, 100 * M + 2 * per_point + lossy, per_point, lossy)
    ref = reference(kappa, a0, gamma, alpha, z_max=Z_MAX, n=N_STEPS, save_every=1, want_traj=True)
    assert (ref["first_bad_step"] == -1).all()
    return dict(kappa=kappa, a0=a0, gamma=gamma, alpha=alpha, rows=ref["traj"])


@pytest.mark.parametrize("save_every", [1, 7, 10])
@pytest.mark.parametrize("lossy", [True, False], ids=["lossy", "lossless"])
@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
@pytest.mark.parametrize("M", [3, 4, 7, 12])
def test_parity(M, per_point, lossy, save_every):
    c = _parity_case(M, per_point, lossy)
    r = run(c["kappa"], n_steps=N_STEPS, z_max=Z_MAX, save_every=save_every, gamma=c["gamma"], alpha=c["alpha"], a0=c["a0"])
    assert r["a_end"].dtype == C64 and r["p_wave_end"].dtype == r["p_wave_max"].dtype == F32
    saved = c["rows"][:, ::save_every]
    err_a = wave_err(r["a_end"], saved[:, -1])
    err_e = power_err(r["p_wave_end"], np.abs(saved[:, -1]) ** 2)
    err_m = power_err(r["p_wave_max"], np.max(np.abs(saved) ** 2, axis=1))
    print(f"M={M} per_point={per_point} lossy={lossy} save_every={save_every}: a_end {err_a:.2e} p_wave_end {err_e:.2e} "
          f"p_wave_max {err_m:.2e}")
    assert (r["first_bad_step"] == -1).all()
    assert err_a < RTOL_F32 and err_e < RTOL_F32 and err_m < RTOL_F32


@pytest.mark.parametrize("M", [4, 12])
def test_the_lossless_promise_changes_no_bit(M):
    """alpha = 0 per point (the host form sets PSA_OPT_LOSSLESS for a broadcast zero only) with and without the flag, and the
    broadcast zero, which carries it."""
    kappa, a0, gamma, _ = rounded_inputs(203, M, 17, lossy=False)
    kw = dict(n_steps=100, z_max=20.0, save_every=7, gamma=gamma, a0=a0, want_traj=True)
    plain = run(kappa, alpha=np.zeros(203, F32), **kw)
    promised = run(kappa, alpha=np.zeros(203, F32), extra_flags=nat.OPT_LOSSLESS, **kw)
    bcast = run(kappa, alpha=0.0, **kw)
    assert np.isfinite(plain["a_end"].view(F32)).all()
    same(plain, promised, KEYS + ("traj",))
    same(plain, bcast, KEYS + ("traj",))


@pytest.mark.parametrize("save_every", [1, 4, 10])
@pytest.mark.parametrize("n_steps", [1, 2, 3, 5, RESYNC - 1, RESYNC, RESYNC + 1, 2 * RESYNC + 1])
def test_loop_edges(n_steps, save_every):
    """One step, odd counts, the re-seed at 16 and one past it, the second one, n_steps < save_every (the only row is z = 0: the
    outputs are a0) and tails that only the check runs."""
    N, M = 70, 4
    kappa, a0, gamma, alpha = rounded_inputs(N, M, 77)
    z_max = 0.5 * n_steps
    r = run(kappa, n_steps=n_steps, z_max=z_max, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    assert (r["first_bad_step"] == -1).all()
    if n_steps < save_every:
        assert np.array_equal(r["a_end"], a0) and np.array_equal(r["p_wave_end"], r["p_wave_max"])
        assert np.max(np.abs(r["p_wave_end"] / np.abs(a0.astype(np.complex128)) ** 2 - 1.0)) < 2e-7
        return
    ref = reference(kappa, a0, gamma, alpha, z_max=z_max, n=n_steps, save_every=save_every)
    err_a, err_e, err_m = (wave_err(r["a_end"], ref["a_end"]), power_err(r["p_wave_end"], ref["p_wave_end"]),
                           power_err(r["p_wave_max"], ref["p_wave_max"]))
    print(f"n_steps={n_steps} save_every={save_every}: {err_a:.2e} {err_e:.2e} {err_m:.2e}")
    assert err_a < RTOL_F32 and err_e < RTOL_F32 and err_m < RTOL_F32


@pytest.mark.parametrize("M", [4, 12])
def test_a_points_result_depends_neither_on_n_nor_on_its_half(M):
    """The first N points of one pool of 203, N = 1 (no scalar kernel: it runs here), the pair, an odd tail, one point short of a
    full wave, the full wave, one past it, and the pool: each equals the pool's run bit for bit, rows included; reversed, every
    point sits in the other half (N even) or in another lane, and changes no bit either.  50 steps pass three seeds."""
    kappa, a0, gamma, alpha = rounded_inputs(203, M, 23)
    kw = dict(n_steps=50, z_max=25.0, save_every=3, want_traj=True)
    keys = KEYS + ("traj",)
    pool = run(kappa, gamma=gamma, alpha=alpha, a0=a0, **kw)
    assert (pool["first_bad_step"] == -1).all() and np.isfinite(pool["traj"].view(F32)).all()
    for N in (1, 2, 3, 127, 128, 129, 203):
        s = slice(0, N)
        head = run(kappa[s], gamma=gamma[s], alpha=alpha[s], a0=a0[s], **kw)
        same(head, {k: pool[k][s] for k in keys}, keys)
        back = run(kappa[s][::-1].copy(), gamma=gamma[s][::-1].copy(), alpha=alpha[s][::-1].copy(), a0=a0[s][::-1].copy(), **kw)
        same({k: back[k][::-1] for k in keys}, head, keys)


@pytest.mark.parametrize("M,N", [(3, 32805), (12, 32805), (3, 65610), (10, 65610), (11, 65610), (12, 65610)])
def test_both_block_sizes_agree_bit_for_bit(M, N):
    """32 805 points are 257 packed waves and a ragged last lane; 65 610 are 513 packed waves, more than half the SIMDs of a
    256-CU device, the size from which the launch takes 256-thread workgroups.  There every instantiation that keeps three
    vectors in LDS runs: M = 10, 11 and 12 take 120, 132 and 144 KiB per workgroup, above the 64 KiB a launch gets unasked.
    PSA_OPT_BLOCK64 forces single-wave workgroups on the same points."""
    kappa, a0, gamma, alpha = rounded_inputs(N, M, 5 + M)
    kw = dict(n_steps=36, z_max=18.0, save_every=10, gamma=gamma, alpha=alpha, a0=a0)
    big = run(kappa, **kw)
    small = run(kappa, extra_flags=nat.OPT_BLOCK64, **kw)
    same(big, small)
    sel = slice(None, None, 257)
    ref = reference(kappa[sel], a0[sel], gamma[sel], alpha[sel], z_max=18.0, n=36, save_every=10)
    err = wave_err(big["a_end"][sel], ref["a_end"])
    print(f"M={M}, {N} points: a_end {err:.2e}")
    assert err < RTOL_F32 and (big["first_bad_step"] == -1).all()


def test_dark_odd_lines_stay_dark():
    """With the odd lines dark every product that lands on an odd line has a dark factor: they stay exactly 0 on the device."""
    N = 203
    kappa, a0, gamma, alpha = rounded_inputs(N, 7, 3)
    a0 = a0.copy()
    a0[:, 1::2] = 0.0
    a0[:, 2] *= 30.0                                       # a strong line among the bright ones
    kw = dict(n_steps=N_STEPS, z_max=Z_MAX, save_every=10, gamma=gamma, alpha=alpha)
    seven = run(kappa, a0=a0, want_traj=True, **kw)
    assert np.all(seven["traj"][:, :, 1::2] == 0) and np.all(seven["p_wave_max"][:, 1::2] == 0)
    assert np.all(seven["a_end"][:, 1::2] == 0) and (seven["first_bad_step"] == -1).all()
    ref = reference(kappa[::7], a0[::7], gamma[::7], alpha[::7], z_max=Z_MAX, n=N_STEPS, save_every=10)
    err = wave_err(seven["a_end"][::7], ref["a_end"])
    print(f"bright lines: {err:.2e}")
    assert err < RTOL_F32 and np.max(np.abs(seven["p_wave_end"][:, ::2] / np.abs(a0[:, ::2]) ** 2 - 1.0)) > 1e-3


FAILING = (10, 21, 40, 41, 130)   # slot 0 of lane 5, slot 1 of lane 10, both halves of lane 20, the odd tail (lane 65 of 131 points)


@pytest.mark.parametrize("M", [4, 12])
def test_failure_index_per_half(M):
    """gamma = 300 overflows within a few steps.  The index of each failing half is the first non-finite row of the kernel's
    own every-step trajectory minus one, whatever the save stride (a tail of 5 steps behind the last row included) and with or
    without PSA_OPT_EXACT_STEP; with the check off it is -1 and the outputs are NaN; the healthy halves and neighbours equal the
    launch without failures bit for bit."""
    N = 131
    kappa, a0, gamma, alpha = rounded_inputs(N, M, 41)
    bad_gamma = gamma.copy()
    bad_gamma[list(FAILING)] = 300.0
    ok = np.ones(N, bool)
    ok[list(FAILING)] = False
    kw = dict(n_steps=45, z_max=9.0, alpha=alpha, a0=a0)
    every = run(kappa, gamma=bad_gamma, save_every=1, want_traj=True, **kw)
    finite = np.isfinite(every["traj"].view(F32).reshape(N, 46, -1)).all(axis=2)
    assert finite[ok].all() and not finite[~ok, -1].any() and finite[:, 0].all()
    want = np.where(ok, -1, np.argmin(finite, axis=1) - 1)
    print("device", every["first_bad_step"][~ok], "first non-finite row - 1", want[~ok])
    assert (want[~ok] >= 0).all() and (want[~ok] < 30).all()
    assert np.array_equal(every["first_bad_step"], want)
    clean = run(kappa, gamma=gamma, save_every=10, **kw)
    assert (clean["first_bad_step"] == -1).all()
    for flags in (dict(), dict(check_nan=False, extra_flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP)):   # without and with PSA_OPT_EXACT_STEP
        got = run(kappa, gamma=bad_gamma, save_every=10, **flags, **kw)
        assert np.array_equal(got["first_bad_step"], want)
        for key in ("a_end", "p_wave_end", "p_wave_max"):
            assert np.array_equal(got[key][ok], clean[key][ok]), key
            assert np.isnan(got[key][~ok].view(F32)).all(), key
    off = run(kappa, gamma=bad_gamma, save_every=10, check_nan=False, **kw)
    assert (off["first_bad_step"] == -1).all()
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(off[key][ok], clean[key][ok]) and np.isnan(off[key][~ok].view(F32)).all(), key


@pytest.mark.parametrize("M", [7, 12])
def test_saved_rows(M):
    """Every saved row at the bar (a full wave's 16-byte stores and the ragged wave's per-half ones); the last row is a_end bit
    for bit, row 0 the input, and the summaries do not depend on the rows being on."""
    c = _parity_case(M, True, True)
    kw = dict(n_steps=N_STEPS, z_max=Z_MAX, save_every=7, gamma=c["gamma"], alpha=c["alpha"], a0=c["a0"])
    r = run(c["kappa"], want_traj=True, **kw)
    assert r["traj"].shape == (203, N_STEPS // 7 + 1, M) and r["traj"].dtype == C64
    err = wave_err(r["traj"], c["rows"][:, ::7])
    print(f"M={M}: rows {err:.2e}")
    assert err < RTOL_F32
    assert np.array_equal(r["traj"][:, 0], c["a0"]) and np.array_equal(r["traj"][:, -1].view(F32), r["a_end"].view(F32))
    same(run(c["kappa"], **kw), r)


def _device_run(torch, kappa, gamma, alpha, a0, *, n_steps, z_max, save_every, flags, traj_ld=None):
    """psa_rk4_comb_f32_dev on torch buffers -> the host entry's dictionary (traj from a [rows][M][ld][2] buffer)."""
    dev = torch.device("cuda:0")
    N, M = kappa.shape
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_k, d_g, d_al = t(kappa.T), t(np.atleast_1d(gamma)), t(np.atleast_1d(alpha))
    d_a0 = t(a0.view(F32).reshape(N, 2 * M).T)
    d_aend = torch.empty((2 * M, N), dtype=torch.float32, device=dev)
    d_we, d_wm = torch.empty((M, N), dtype=torch.float32, device=dev), torch.empty((M, N), dtype=torch.float32, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    rows = n_steps // save_every + 1
    d_traj = None if traj_ld is None else torch.full((rows, M, traj_ld, 2), -7.0, dtype=torch.float32, device=dev)
    nat.comb_device(stream=torch.cuda.current_stream().cuda_stream, n_lines=M, n_points=N, n_steps=n_steps, z_max=z_max,
                    save_every=save_every, d_kappa_soa=d_k.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                    d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(), d_p_wave_end_soa=d_we.data_ptr(),
                    d_p_wave_max_soa=d_wm.data_ptr(), d_first_bad=d_bad.data_ptr(),
                    d_traj_soa=(0 if d_traj is None else d_traj.data_ptr()), dtype=F32)
    torch.cuda.synchronize()
    out = dict(a_end=np.ascontiguousarray(d_aend.cpu().numpy().T).view(C64), p_wave_end=d_we.cpu().numpy().T,
               p_wave_max=d_wm.cpu().numpy().T, first_bad_step=d_bad.cpu().numpy(), traj=None, pad=None)
    if d_traj is not None:
        full = d_traj.cpu().numpy()                                          # [rows][M][ld][2]
        out["traj"] = np.ascontiguousarray(full[:, :, :N].transpose(2, 0, 1, 3)).view(C64)[..., 0]
        out["pad"] = full[:, :, N:]
    return out


@pytest.mark.parametrize("N,M,n_steps", [(300, 12, 40), (262144, 3, 5)])
def test_device_entry_with_padded_rows_equals_the_host_entry(N, M, n_steps):
    """PSA_OPT_TRAJ_LD on the `_dev` form: the rows' regions have the leading dimension psa_traj_ld(N, 4).  300 points need no
    padding (the flag changes nothing), 262 144 points would put the regions 2 MiB apart and are padded by 544 points.  The
    `_dev` form with the flag, the dense one and the host form (which pads internally) agree bit for bit, and the padding is
    never written."""
    torch = pytest.importorskip("torch")
    ld = nat.traj_ld(N, F32)
    assert ld == (N + 544 if N == 262144 else N)
    kappa, a0, gamma, alpha = rounded_inputs(N, M, 13)
    kw = dict(n_steps=n_steps, z_max=0.5 * n_steps, save_every=2)
    dense = _device_run(torch, kappa, gamma, alpha, a0, flags=nat.OPT_CHECK_NAN, traj_ld=N, **kw)
    padded = _device_run(torch, kappa, gamma, alpha, a0, flags=nat.OPT_CHECK_NAN | nat.OPT_TRAJ_LD, traj_ld=ld, **kw)
    host = run(kappa, gamma=gamma, alpha=alpha, a0=a0, want_traj=True, **kw)
    keys = KEYS + ("traj",)
    same(dense, padded, keys)
    same(dense, host, keys)
    assert dense["traj"].shape == (N, n_steps // 2 + 1, M) and np.all(padded["pad"] == -7.0) and padded["pad"].shape[2] == ld - N
    assert (host["first_bad_step"] == -1).all() and np.isfinite(host["traj"].view(F32)).all()


def test_two_blocks_on_one_device_equal_one_launch_and_sit_next_to_float64():
    N, M = 203, 6
    kappa, a0, gamma, alpha = comb_np.random_inputs(N, M, 31)
    kw = dict(z_max=50.0, n_steps=500, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    one = sweep.rk4_sweep_comb(kappa, dtype=F32, **kw)
    two = sweep.rk4_sweep_comb(kappa, dtype=F32, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (N, 51, M) and one.traj.dtype == C64 and one.p_wave_end.dtype == F32
    assert np.array_equal(one.p_wave_in, np.abs(a0.astype(C64)) ** 2) and (one.first_bad_step == -1).all()
    # next to the float64 call on the unrounded inputs: the kernel's bar is 1e-4 of the point's largest line A_max on every
    # amplitude, so a line of at least 0.1 A_max has its power within 2e-3 + 1e-6 of itself (0.0087 dB), and the total power,
    # sum A_m^2 with sum A_m A_max <= sqrt(M) sum A_m^2, within 2e-4 sqrt(M) of itself
    ref = sweep.rk4_sweep_comb(kappa, **kw)
    assert wave_err(one.a_end, ref.a_end) < RTOL_F32
    p0 = np.abs(a0) ** 2
    g32, g64 = one.line_gain(p0, mode="end"), ref.line_gain(p0, mode="end")
    strong = ref.p_wave_end >= 0.01 * ref.p_wave_end.max(axis=1, keepdims=True)
    d_gain = float(np.max(np.abs(g32 - g64)[strong]))
    d_total = float(np.max(np.abs(one.total_power() / ref.total_power() - 1.0)))
    print(f"line_gain on the strong lines {d_gain:.2e} dB, total_power {d_total:.2e}")
    assert strong.sum() >= 2 * N and d_gain < 0.0087 and d_total < 2e-4 * np.sqrt(M)
    assert np.array_equal(np.isnan(g32), np.isnan(g64))


def test_gain_driver_next_to_float64(golden):
    """scan_comb_gain(dtype=np.float32) beside the float64 driver on two 0.3 W pumps 400 GHz apart on an eight-line 200 GHz grid
    with a seed between them: every lit line within 1e-3 dB, a dark line NaN in both."""
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    cfg = config.custom_simulation_config(z_max=300.0, dz=0.2)
    p = np.zeros((5, 8))
    p[:, 3] = p[:, 5] = 0.3
    p[:, 4] = 10.0 ** np.arange(-7, -2)
    kw = dict(cfg=cfg, lambda_center_m=1550e-9, line_spacing=2.0 * np.pi * 200e9, p_lines=p, gamma=0.0115, alpha=1e-4, dispersion=d,
              gain_mode="end")
    f64 = scan_mismtach.scan_comb_gain(**kw)
    f32 = scan_mismtach.scan_comb_gain(dtype=F32, **kw)
    assert f32["result"].a_end.dtype == C64 and f32["p_end"].dtype == F32 and np.array_equal(f32["kappa"], f64["kappa"])
    lit = p > 0
    assert np.isnan(f32["gain"][~lit]).all() and np.isnan(f64["gain"][~lit]).all()
    assert np.isfinite(f32["gain"][lit]).all() and (f32["first_bad_step"] == -1).all()
    worst = float(np.max(np.abs(f32["gain"][lit] - f64["gain"][lit])))
    print(f"lit lines: float32 against float64 gain {worst:.2e} dB")
    assert worst < 1e-3
    assert np.all(f32["p_end"][:, [1, 7]] > 1e-9)           # the cascaded pump products come up in float32 too
