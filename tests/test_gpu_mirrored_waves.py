"""The mirrored z-loop of the one-lane float64 four-wave kernel: a wave whose live lanes all start
with A2 == A1 and A4 == A3 bit for bit, all finite, integrates waves 1 and 3 only and writes the full record from them.

The loop must return the bits of the general loop.  Both run inside ONE launch here: a wave of mirrored points next to a wave
that holds the same points with an asymmetric lane or two, which sends it through the general loop.  Every case forces
PSA_OPT_ONE_LANE (sweeps this small would otherwise take two or four lanes per point)."""
import numpy as np
import pytest

import psa_amd._native as nat

pytestmark = pytest.mark.gpu

GAMMA, ALPHA = 0.0115, 1.15e-4                       # the headline workload's constants
I_PUMP, I_IDLER = 5, 40                              # the two asymmetric lanes of the general wave
SHARED = np.array([k for k in range(64) if k not in (I_PUMP, I_IDLER)])
# the static FP64 counts of the two z-loops per RK4 step, general and mirrored (tools/isa_loop_stats.py --top=2 on the
# headline instantiation, profiles/mirrored_waves.log; the hand count of the mirrored step is 186, the compiler shares
# y*y between |A|^2 and A*A in each of its eight squares)
STEP_GENERAL, STEP_MIRRORED = 298, 178


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype.kind in "fc" else x


def same_bits(a, b):
    """array_equal on the bit patterns: +0 / -0 differ, equal NaNs match"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ulp_off(z):
    return complex(np.nextafter(z.real, np.inf), z.imag)


def _three_waves():
    """165 points: wave 0 mirrored, wave 1 the same 64 parameter sets with two asymmetric lanes, wave 2 = 37 mirrored points
    (the first 37 sets again).  Amplitudes carry non-zero phases."""
    rng = np.random.default_rng(20261018)
    db64, gam64, al64 = rng.uniform(-0.05, 0.05, 64), rng.uniform(5e-3, 2e-2, 64), rng.uniform(5e-5, 3e-4, 64)
    pump = np.sqrt(rng.uniform(0.2, 0.8, 64)) * np.exp(1j * rng.uniform(-3.1, 3.1, 64))
    side = np.sqrt(rng.uniform(1e-6, 1e-3, 64)) * np.exp(1j * rng.uniform(-3.1, 3.1, 64))
    a64 = np.column_stack([pump, pump, side, side])
    pick = np.r_[0:64, 0:64, 0:37]
    a0 = a64[pick].copy()
    a0[64 + I_PUMP, 1] = ulp_off(a0[64 + I_PUMP, 0])         # A2 one ulp off A1
    a0[64 + I_IDLER, 3] = 1.5 * a0[64 + I_IDLER, 2]          # A4 != A3
    return db64[pick], gam64[pick], al64[pick], a0


KEYS = ("a_end", "p_end", "p_max", "first_bad_step")
CHECKS = [pytest.param(dict(check_nan=False), id="none"), pytest.param(dict(check_nan=True, exact_step=False), id="block"),
          pytest.param(dict(check_nan=True, exact_step=True), id="exact")]


@pytest.mark.parametrize("block", [pytest.param(0, id="wg256"), pytest.param(nat.OPT_BLOCK64, id="wg64")])
@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("lossy", [pytest.param(True, id="lossy"), pytest.param(False, id="lossless")])
@pytest.mark.parametrize("se,traj", [(7, False), (7, True), (64, False), (64, True), (1, True)])
def test_both_loops_give_the_same_bits(se, traj, lossy, check, block):
    """200 steps: save_every 7 leaves a tail of 4 and crosses the re-seeds at 64, 128 and 192; 64 saves on the seed grid;
    1 with a trajectory is the dedicated every-step loop."""
    db, gam, al, a0 = _three_waves()
    kw = dict(n_steps=200, z_max=20.0, save_every=se, gamma=gam, alpha=(al if lossy else 0.0), a0=a0,
              extra_flags=nat.OPT_ONE_LANE | block, **check)
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
        assert same_bits(v[SHARED], v[64 + SHARED]), k       # mirrored loop == general loop
        assert same_bits(v[128:165], v[0:37]), k             # the partial wave == the full one
    mirrored = np.r_[0:64, 64 + SHARED, 128:165]
    for v in [got["a_end"]] + ([got["traj"]] if traj else []):
        assert same_bits(v[mirrored][..., 1], v[mirrored][..., 0]) and same_bits(v[mirrored][..., 3], v[mirrored][..., 2])
    if "p_wave_end" in outs:
        for v in (outs["p_wave_end"], outs["p_wave_max"]):
            assert same_bits(v[mirrored][:, 1], v[mirrored][:, 0]) and same_bits(v[mirrored][:, 3], v[mirrored][:, 2])


def test_failing_points_replay_the_mirrored_step(golden):
    """Golden G9's per-point gamma ladder (first_bad_step [1, 1, 1, 2, 3, 4, 5, -1]) in lanes 0..7 of a mirrored wave and of
    a wave with one asymmetric lane; the other lanes hold the ladder's healthy gamma."""
    g = golden("G9")
    want = g["first_bad_step"]
    a0 = np.tile(np.sqrt(g["p_in"]).astype(complex), (128, 1))
    a0[64 + 20, 1] = ulp_off(a0[64 + 20, 0])
    gam = np.full(128, g["gammas"][-1])
    gam[0:8] = gam[64:72] = g["gammas"]
    db = np.full(128, float(g["dbeta"]))
    kw = dict(n_steps=1000, z_max=float(g["z_max"]), save_every=10, gamma=gam, alpha=0.0, a0=a0, extra_flags=nat.OPT_ONE_LANE)
    exact = nat.sweep_host(db, check_nan=True, exact_step=True, **kw)
    assert np.array_equal(exact["first_bad_step"][0:8], want)
    assert np.array_equal(exact["first_bad_step"][64:72], want)
    assert (exact["first_bad_step"][8:64] == -1).all() and (exact["first_bad_step"][72:128] == -1).all()
    block = nat.sweep_host(db, check_nan=True, exact_step=False, **kw)
    assert np.array_equal(block["first_bad_step"][0:8], np.where(want >= 0, 9, -1))
    assert np.array_equal(block["first_bad_step"][0:64], block["first_bad_step"][64:128])
    # the healthy point next to seven replays: the bits it has when it runs alone
    solo = nat.sweep_host(db[7:8], check_nan=True, exact_step=True, **{**kw, "gamma": gam[7:8], "a0": a0[7:8]})
    for k in KEYS:
        assert same_bits(exact[k][7:8], solo[k]) and same_bits(exact[k][64 + 7:64 + 8], solo[k]), k
        assert same_bits(block[k][7:8], solo[k]), k


def _against_a_general_wave(a0_64):
    """points 0..63 = a0_64; points 64..127 the same with lane I_IDLER asymmetric -> equal bits everywhere else"""
    rng = np.random.default_rng(5)
    db64 = rng.uniform(-0.05, 0.05, 64)
    a0 = np.concatenate([a0_64, a0_64])
    a0[64 + I_IDLER, 3] = 1.5 * a0[64 + I_IDLER, 2]
    got = nat.sweep_host(np.r_[db64, db64], n_steps=200, z_max=20.0, save_every=7, gamma=GAMMA, alpha=ALPHA, a0=a0,
                         want_traj=True, check_nan=True, exact_step=True, extra_flags=nat.OPT_ONE_LANE)
    keep = np.array([k for k in range(64) if k != I_IDLER])
    for k in KEYS + ("traj",):
        assert same_bits(got[k][keep], got[k][64 + keep]), k
    return got


def test_a_signed_zero_keeps_the_wave_in_the_general_loop():
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(complex), (64, 1))
    a0[3, 0], a0[3, 1] = complex(0.0, 0.7), complex(-0.0, 0.7)       # x1 = +0.0, x2 = -0.0: equal values, different bits
    assert a0[3, 0] == a0[3, 1] and not same_bits(a0[3, 0:1], a0[3, 1:2])
    got = _against_a_general_wave(a0)
    assert (got["first_bad_step"] == -1).all()


def test_a_nan_keeps_the_wave_in_the_general_loop():
    a0 = np.tile(np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(complex), (64, 1))
    a0[9, 2] = a0[9, 3] = complex(np.nan, 1e-3)                      # mirrored bit for bit, but not finite
    got = _against_a_general_wave(a0)
    assert got["first_bad_step"][9] == got["first_bad_step"][64 + 9] == 0
    assert (np.delete(got["first_bad_step"], [9, 64 + 9]) == -1).all()


def test_the_mirrored_loop_is_taken():
    """Bit-identity cannot show which loop ran, so time it: 65 536 points x 2 000 steps with the headline constants on the
    device API, kernel time from events around the call, median of five launches; mirrored inputs against
    p_in = (0.5, 0.4, 1e-5, 1e-5).  The bound is the midpoint between 1 and the ratio of the two loops' static instruction
    counts: the margin is for the clock under the denser loop."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    N, n = 65_536, 2000
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)   # noqa: E731
    d_db, d_g, d_al = t(np.linspace(-0.05, 0.05, N)), t([GAMMA]), t([ALPHA])
    d_aend = torch.empty((8, N), dtype=torch.float64, device=dev)
    d_pe, d_pm = torch.empty(N, dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    flags = (nat.BCAST_GAMMA | nat.BCAST_ALPHA | nat.BCAST_A0 | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_ONE_LANE)

    def median_ms(p_in):
        d_a0 = t(np.sqrt(np.asarray(p_in)).astype(complex).view(np.float64).reshape(8, 1))
        times = []
        for k in range(6):                                           # the first launch warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.sweep_device(stream=torch.cuda.current_stream().cuda_stream, n_waves=4, n_points=N, n_steps=n, z_max=20.0,
                             save_every=10, d_dbeta=d_db.data_ptr(), d_dbeta2=0, d_gamma=d_g.data_ptr(),
                             d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                             d_p_end=d_pe.data_ptr(), d_p_max=d_pm.data_ptr(), d_first_bad=d_bad.data_ptr())
            e1.record()
            e1.synchronize()
            if k:
                times.append(e0.elapsed_time(e1))
        assert (d_bad == -1).all()
        return float(np.median(times))

    mirrored = median_ms([0.5, 0.5, 1e-5, 1e-5])
    general = median_ms([0.5, 0.4, 1e-5, 1e-5])
    bound = 0.5 * (1.0 + STEP_MIRRORED / STEP_GENERAL)
    print(f"mirrored {mirrored:.4f} ms, asymmetric {general:.4f} ms, ratio {mirrored / general:.4f} (bound {bound:.4f})")
    assert mirrored / general < bound
