"""The mirrored z-loop of the packed float32 four-wave kernel: a wave whose live lanes all start, in BOTH of
their points, with A2 == A1 and A4 == A3 bit for bit, all finite, integrates waves 1 and 3 only and writes the full record
from them.

The loop must return the bits of the general loop.  Both run inside ONE launch here: a wave of mirrored points (128 points,
two per lane) next to a wave that holds the same points with an asymmetric point or two, which sends it through the general
loop.  Every case forces PSA_OPT_F32_PACKED."""
import numpy as np
import pytest

import psa_amd._native as nat

pytestmark = pytest.mark.gpu

F32 = dict(dtype=np.float32, extra_flags=nat.OPT_F32_PACKED)
GAMMA, ALPHA = 0.0115, 1.15e-4
W = 128                                              # points of one packed wave
I_PUMP, I_IDLER = 10, 81                             # the asymmetric points of the general wave: lane 5 slot 0, lane 40 slot 1
SHARED = np.array([k for k in range(W) if k not in (I_PUMP, I_IDLER)])
TAIL = 75                                            # points of the third wave: lane 37 holds one point, lanes 38.. none
# the static packed-instruction counts of the two z-loops per RK4 step and point pair, general and mirrored
# (tools/isa_loop_stats.py --top=2 on rk4_sweep_pk_kernel<4, 1, false, 256, false>: 656 and 376 per two-step trip,
# profiles/mirrored_f32.log)
STEP_GENERAL, STEP_MIRRORED = 328, 188


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.kind in "fc" else x


def same_bits(a, b):
    """array_equal on the bit patterns: +0 / -0 differ, equal NaNs match"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ulp_off(z):
    return np.complex64(complex(np.nextafter(np.float32(z.real), np.float32(np.inf)), z.imag))


def _three_waves():
    """331 points: wave 0 mirrored, wave 1 the same 128 parameter sets with two asymmetric points, wave 2 = 75 mirrored points
    (the first 75 sets again: an odd tail and past-the-end lanes).  Amplitudes carry non-zero phases."""
    rng = np.random.default_rng(20261018)
    db, gam, al = rng.uniform(-0.05, 0.05, W), rng.uniform(5e-3, 2e-2, W), rng.uniform(5e-5, 3e-4, W)
    pump = np.sqrt(rng.uniform(0.2, 0.8, W)) * np.exp(1j * rng.uniform(-3.1, 3.1, W))
    side = np.sqrt(rng.uniform(1e-6, 1e-3, W)) * np.exp(1j * rng.uniform(-3.1, 3.1, W))
    aw = np.column_stack([pump, pump, side, side]).astype(np.complex64)
    pick = np.r_[0:W, 0:W, 0:TAIL]
    a0 = aw[pick].copy()
    a0[W + I_PUMP, 1] = ulp_off(a0[W + I_PUMP, 0])           # A2 one ulp off A1
    a0[W + I_IDLER, 3] = np.complex64(1.5) * a0[W + I_IDLER, 2]   # A4 != A3
    return db[pick], gam[pick], al[pick], a0


KEYS = ("a_end", "p_end", "p_max", "first_bad_step")
CHECKS = [pytest.param(dict(check_nan=False), id="none"), pytest.param(dict(check_nan=True, exact_step=False), id="block"),
          pytest.param(dict(check_nan=True, exact_step=True), id="exact")]


@pytest.mark.parametrize("block", [pytest.param(0, id="wg256"), pytest.param(nat.OPT_BLOCK64, id="wg64")])
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("se,traj", [(7, False), (7, True), (16, False), (16, True), (1, True)])
def test_both_loops_give_the_same_bits(se, traj, check, block):
    """200 steps: save_every 7 leaves a tail of 4 and crosses the seeds and folds at every 16; 16 saves on the seed grid;
    1 with a trajectory is the dedicated every-step loop."""
    db, gam, al, a0 = _three_waves()
    kw = dict(n_steps=200, z_max=20.0, save_every=se, gamma=gam, alpha=al, a0=a0, dtype=np.float32,
              extra_flags=nat.OPT_F32_PACKED | block, **check)
    got = nat.sweep_host(db, want_traj=traj, **kw)
    outs = {k: got[k] for k in KEYS + (("traj",) if traj else ())}
    if not traj and not block:                               # the per-wave summary: no trajectory, 256-thread workgroups
        ws = nat.sweep_host(db, wave_summary=True, **kw)
        for k in KEYS:
            assert same_bits(ws[k], got[k]), k
        outs.update(p_wave_end=ws["p_wave_end"], p_wave_max=ws["p_wave_max"])
        assert same_bits(ws["p_wave_end"][:, 2], ws["p_end"]) and same_bits(ws["p_wave_max"][:, 2], ws["p_max"])
    assert (got["first_bad_step"] == -1).all() and np.isfinite(got["a_end"]).all()
    for k, v in outs.items():
        assert same_bits(v[SHARED], v[W + SHARED]), k        # mirrored loop == general loop
        assert same_bits(v[2 * W:2 * W + TAIL], v[0:TAIL]), k   # the partial wave == the full one
    mirrored = np.r_[0:W, W + SHARED, 2 * W:2 * W + TAIL]
    for v in [got["a_end"]] + ([got["traj"]] if traj else []):
        assert same_bits(v[mirrored][..., 1], v[mirrored][..., 0]) and same_bits(v[mirrored][..., 3], v[mirrored][..., 2])
    if "p_wave_end" in outs:
        for v in (outs["p_wave_end"], outs["p_wave_max"]):
            assert same_bits(v[mirrored][:, 1], v[mirrored][:, 0]) and same_bits(v[mirrored][:, 3], v[mirrored][:, 2])


def test_failing_points_fail_at_the_same_step(golden):
    """Golden G9's per-point gamma ladder in lanes 0..7 of a mirrored wave and of a wave with one asymmetric point (entry j in
    lane j, slots alternating); the other points hold the ladder's healthy gamma.  Float32 need not fail where G9's float64
    does, so the condition on the ladder -- at least three points fail, at least one does not -- is asserted on the GENERAL
    loop, and the mirrored loop must then agree with it point for point."""
    g = golden("G9")
    ladder = np.array([2 * j + (j % 2) for j in range(8)])
    a0 = np.tile(np.sqrt(g["p_in"]).astype(np.complex64), (2 * W, 1))
    a0[W + 41, 1] = ulp_off(a0[W + 41, 0])
    gam = np.full(2 * W, g["gammas"][-1])
    gam[ladder] = gam[W + ladder] = g["gammas"]
    db = np.full(2 * W, float(g["dbeta"]))
    kw = dict(n_steps=1000, z_max=float(g["z_max"]), save_every=10, gamma=gam, alpha=0.0, a0=a0, **F32)
    exact = nat.sweep_host(db, check_nan=True, exact_step=True, **kw)
    block = nat.sweep_host(db, check_nan=True, exact_step=False, **kw)
    fb = exact["first_bad_step"]
    print("first_bad_step of the ladder, general wave:", fb[W + ladder], " mirrored wave:", fb[ladder])
    assert (fb[W + ladder] >= 0).sum() >= 3 and (fb[W + ladder] == -1).sum() >= 1
    others = np.setdiff1d(np.arange(W), ladder)
    assert (fb[others] == -1).all() and (fb[W + others] == -1).all()
    assert np.array_equal(fb[0:W], fb[W:2 * W])
    assert np.array_equal(block["first_bad_step"][0:W], block["first_bad_step"][W:2 * W])
    assert np.array_equal(block["first_bad_step"][0:W], np.where(fb[0:W] >= 0, fb[0:W] // 10 * 10 + 9, -1))
    healthy = ladder[fb[W + ladder] == -1]
    for k in KEYS:
        assert same_bits(exact[k][healthy], exact[k][W + healthy]), k
        assert same_bits(block[k][healthy], block[k][W + healthy]) and same_bits(block[k][healthy], exact[k][healthy]), k


def _against_a_general_wave(a0_w, **over):
    """points 0..127 = a0_w; points 128..255 the same with point I_IDLER asymmetric -> equal bits everywhere else"""
    rng = np.random.default_rng(5)
    dbw = rng.uniform(-0.05, 0.05, W)
    a0 = np.concatenate([a0_w, a0_w]).astype(np.complex64)
    a0[W + I_IDLER, 3] = np.complex64(1.5) * a0[W + I_IDLER, 2]
    kw = dict(n_steps=200, z_max=20.0, save_every=7, gamma=GAMMA, alpha=ALPHA, a0=a0, want_traj=True, check_nan=True,
              exact_step=True, **F32)
    kw.update(over)
    got = nat.sweep_host(np.r_[dbw, dbw], **kw)
    keep = np.array([k for k in range(W) if k != I_IDLER])
    for k in KEYS + ("traj",):
        assert same_bits(got[k][keep], got[k][W + keep]), k
    return got


def test_a_signed_zero_keeps_the_wave_in_the_general_loop():
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(np.complex64), (W, 1))
    a0[3, 0], a0[3, 1] = complex(0.0, 0.7), complex(-0.0, 0.7)       # x1 = +0.0, x2 = -0.0: equal values, different bits
    assert a0[3, 0] == a0[3, 1] and not same_bits(a0[3, 0:1], a0[3, 1:2])
    got = _against_a_general_wave(a0)
    assert (got["first_bad_step"] == -1).all()


def test_a_nan_keeps_the_wave_in_the_general_loop():
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(np.complex64), (W, 1))
    a0[9, 2] = a0[9, 3] = complex(np.nan, 1e-3)                      # mirrored bit for bit, but not finite
    got = _against_a_general_wave(a0)
    assert got["first_bad_step"][9] == got["first_bad_step"][W + 9] == 0
    assert (np.delete(got["first_bad_step"], [9, W + 9]) == -1).all()


def test_small_magnitudes_give_the_same_bits():
    """sidebands of 1e-20 ... 1e-23: every x*y of A3*A3 (1e-40 ... 1e-46) is subnormal in float32 -- or zero -- where the
    folded stage multiplies the un-doubled product by the doubled phase factor"""
    rng = np.random.default_rng(11)
    pump = np.sqrt(rng.uniform(0.2, 0.8, W)) * np.exp(1j * rng.uniform(-3.1, 3.1, W))
    side = 10.0 ** rng.uniform(-23, -20, W) * np.exp(1j * rng.uniform(-3.1, 3.1, W))
    a0 = np.column_stack([pump, pump, side, side]).astype(np.complex64)
    got = _against_a_general_wave(a0)
    assert (got["first_bad_step"] == -1).all() and (np.abs(got["a_end"][:, 2]) > 0).all()


def test_the_mirrored_loop_is_taken():
    """Bit-identity cannot show which loop ran, so time it: 131 072 points x 2 000 steps on the device API, kernel time from
    events around the call, median of five launches after a warm-up; the benchmark's mirrored p_in against
    (0.1, 0.08, 1e-7, 1e-7).  The bound is the midpoint between 1 and the ratio of the two loops' static instruction counts:
    the margin is for the clock under the denser loop."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    N, n = 131_072, 2000
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)   # noqa: E731
    d_db, d_g, d_al = t(np.linspace(-0.05, 0.05, N)), t([GAMMA]), t([ALPHA])
    d_aend = torch.empty((8, N), dtype=torch.float32, device=dev)
    d_pe, d_pm = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    flags = nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.OPT_CHECK_NAN | nat.OPT_F32_PACKED

    def median_ms(p_in):
        d_a0 = t(np.sqrt(np.asarray(p_in)).astype(np.complex64).view(np.float32).reshape(8, 1))
        times = []
        for k in range(6):                                           # the first launch warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.sweep_device(stream=torch.cuda.current_stream().cuda_stream, n_waves=4, n_points=N, n_steps=n, z_max=20.0,
                             save_every=10, d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(),
                             d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                             d_p_end=d_pe.data_ptr(), d_p_max=d_pm.data_ptr(), d_first_bad=d_bad.data_ptr(), dtype=np.float32)
            e1.record()
            e1.synchronize()
            if k:
                times.append(e0.elapsed_time(e1))
        assert (d_bad == -1).all()
        return float(np.median(times))

    mirrored = median_ms([0.1, 0.1, 1e-7, 1e-7])
    general = median_ms([0.1, 0.08, 1e-7, 1e-7])
    bound = 0.5 * (1.0 + STEP_MIRRORED / STEP_GENERAL)
    print(f"mirrored {mirrored:.4f} ms, asymmetric {general:.4f} ms, ratio {mirrored / general:.4f} (bound {bound:.4f})")
    assert mirrored / general < bound
