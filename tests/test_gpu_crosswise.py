"""The crosswise four-wave stage on the GPU: the general z-loops of the one-lane float64
kernel and of the float32 kernels pair the triple products crosswise, so that waves 1 / 2 and waves 3 / 4 are one expression
with the partner's operands exchanged, and the mirrored z-loops are those loops with the duplicates removed.

* exchange symmetry: a launch with waves 1 <-> 2 and 3 <-> 4 exchanged returns the permuted record bit for bit;
* oracle parity of mirrored and asymmetric points at the bars of record;
* the two-lane layout hands mirrored waves to the same mirrored loop: the record does not depend on the layout there;
* the mirrored loop's share of the general loop's time is what the two loops' instruction counts say.

Bit-identity of the mirrored and the general loop is tests/test_gpu_mirrored_waves.py and test_gpu_mirrored_packed.py."""
import numpy as np
import pytest

import psa_amd._native as nat
from conftest import RTOL_F32, RTOL_F64, rel_err

pytestmark = pytest.mark.gpu

GAMMA, ALPHA = 0.0115, 1.15e-4
EXCHANGE = [1, 0, 3, 2]                              # waves after A1 <-> A2, A3 <-> A4
# the timing bound's constants: FP64 instructions per RK4 step of the general loop and the count the crosswise mirrored step was
# specified with (the built loop has 154: E2 = E + E for stage 3 stays; the bound is kept at the stricter figure)
STEP_GENERAL, STEP_MIRRORED = 298, 152


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.real.dtype.itemsize]) if x.dtype.kind in "fc" else x


def same_bits(a, b):
    """array_equal on the bit patterns: +0 / -0 differ, equal NaNs match"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _asymmetric_points(N, cdt):
    """random pumps and sidebands with phases, per-point gamma, alpha and dbeta: no point is mirrored"""
    rng = np.random.default_rng(20261018 + N)
    db, gam, al = rng.uniform(-0.05, 0.05, N), rng.uniform(5e-3, 2e-2, N), rng.uniform(5e-5, 3e-4, N)
    p = np.column_stack([rng.uniform(0.2, 0.8, (N, 2)), 10 ** rng.uniform(-6, -3, (N, 2))])
    a0 = (np.sqrt(p) * np.exp(1j * rng.uniform(-3.1, 3.1, (N, 4)))).astype(cdt)
    assert np.all(a0[:, 0] != a0[:, 1]) and np.all(a0[:, 2] != a0[:, 3])
    return db, gam, al, a0


def _exchange_case(N, dtype, layout, lossy, block):
    """Two launches, the second with the partners exchanged: a_end and the trajectory permuted and equal in every bit, the
    per-wave summary likewise; p_end / p_max follow the signal (wave 3), which after the exchange is the first run's idler."""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    db, gam, al, a0 = _asymmetric_points(N, cdt)
    kw = dict(n_steps=200, z_max=20.0, save_every=7, gamma=gam, alpha=(al if lossy else 0.0), dtype=dtype)
    one = nat.sweep_host(db, a0=a0, want_traj=True, extra_flags=layout | block, **kw)
    two = nat.sweep_host(db, a0=a0[:, EXCHANGE], want_traj=True, extra_flags=layout | block, **kw)
    assert (one["first_bad_step"] == -1).all() and (two["first_bad_step"] == -1).all() and np.isfinite(one["a_end"]).all()
    assert same_bits(two["a_end"], one["a_end"][:, EXCHANGE])
    assert same_bits(two["traj"], one["traj"][:, :, EXCHANGE])
    assert same_bits(one["traj"][:, -1, :], one["a_end"])
    # the per-wave summary exists without trajectory in 256-thread workgroups; the arithmetic does not depend on either
    ws1 = nat.sweep_host(db, a0=a0, wave_summary=True, extra_flags=layout, **kw)
    ws2 = nat.sweep_host(db, a0=a0[:, EXCHANGE], wave_summary=True, extra_flags=layout, **kw)
    for k in ("p_wave_end", "p_wave_max"):
        assert same_bits(ws2[k], ws1[k][:, EXCHANGE]), k
    assert same_bits(ws1["a_end"], one["a_end"]) and same_bits(ws2["a_end"], two["a_end"])
    assert same_bits(one["p_end"], ws1["p_wave_end"][:, 2]) and same_bits(one["p_max"], ws1["p_wave_max"][:, 2])
    assert same_bits(two["p_end"], ws1["p_wave_end"][:, 3]) and same_bits(two["p_max"], ws1["p_wave_max"][:, 3])


BLOCKS = [pytest.param(0, id="wg256"), pytest.param(nat.OPT_BLOCK64, id="wg64")]
LOSS = [pytest.param(True, id="lossy"), pytest.param(False, id="lossless")]


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lossy", LOSS)
def test_exchanging_the_partners_permutes_the_record_float64(lossy, block):
    """128 asymmetric points in the general loop of the one-lane kernel; 200 steps, save_every 7: a tail of 4, re-seeds at 64,
    128 and 192 between saved rows."""
    _exchange_case(128, np.float64, nat.OPT_ONE_LANE, lossy, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lossy", LOSS)
@pytest.mark.parametrize("layout", [pytest.param(nat.OPT_F32_SCALAR, id="scalar"), pytest.param(nat.OPT_F32_PACKED, id="packed")])
def test_exchanging_the_partners_permutes_the_record_float32(layout, lossy, block):
    """256 points: two waves of the packed kernel (two points per lane), four of the scalar one"""
    _exchange_case(256, np.float32, layout, lossy, block)


@pytest.mark.parametrize("lossy", LOSS)
def test_mirrored_and_asymmetric_points_match_the_oracle(oracle, lossy):
    """192 points, 2 000 steps: 64 mirrored points (one full wave of the one-lane kernel: the mirrored loop), 128 asymmetric
    ones (the general loop); the float32 kernels take the same points (a packed wave holds 128).  Float64 at RTOL_F64 in the
    one-lane layout, float32 scalar and packed at RTOL_F32."""
    rng = np.random.default_rng(192)
    N = 192
    db, gam = rng.uniform(-0.05, 0.05, N), rng.uniform(5e-3, 2e-2, N)
    al = rng.uniform(5e-5, 3e-4, N) if lossy else 0.0
    a0 = np.sqrt(rng.uniform([0.3, 0.3, 1e-6, 1e-6], [0.6, 0.6, 1e-4, 1e-4], (N, 4))) * np.exp(1j * rng.uniform(-3, 3, (N, 4)))
    a0[:64, 1], a0[:64, 3] = a0[:64, 0], a0[:64, 2]
    a0_32 = a0.astype(np.complex64)
    kw = dict(n_steps=2000, z_max=200.0, save_every=10, gamma=gam, alpha=al)
    ref = oracle.sweep(db, z_max=200.0, n=2000, save_every=10, gamma=gam, alpha=al, a0=a0)
    ref32 = oracle.sweep(db, z_max=200.0, n=2000, save_every=10, gamma=gam, alpha=al, a0=a0_32.astype(complex))
    assert (ref["first_bad_step"] == -1).all()
    got = nat.sweep_host(db, a0=a0, extra_flags=nat.OPT_ONE_LANE, **kw)
    errs = [rel_err(got[k], ref[k]) for k in ("a_end", "p_end", "p_max")]
    print(f"float64 one lane: a_end {errs[0]:.2e} p_end {errs[1]:.2e} p_max {errs[2]:.2e}")
    assert max(errs) < RTOL_F64 and (got["first_bad_step"] == -1).all()
    assert same_bits(got["a_end"][:64, 1], got["a_end"][:64, 0]) and same_bits(got["a_end"][:64, 3], got["a_end"][:64, 2])
    for name, layout in (("scalar", nat.OPT_F32_SCALAR), ("packed", nat.OPT_F32_PACKED)):
        g32 = nat.sweep_host(db, a0=a0_32, dtype=np.float32, extra_flags=layout, **kw)
        errs = [rel_err(g32["a_end"].astype(complex), ref32["a_end"]), rel_err(g32["p_end"].astype(float), ref32["p_end"]),
                rel_err(g32["p_max"].astype(float), ref32["p_max"])]
        print(f"float32 {name}: a_end {errs[0]:.2e} p_end {errs[1]:.2e} p_max {errs[2]:.2e}")
        assert max(errs) < RTOL_F32 and (g32["first_bad_step"] == -1).all()


CHECKS = [pytest.param(dict(check_nan=False), id="none"), pytest.param(dict(check_nan=True, exact_step=False), id="block"),
          pytest.param(dict(check_nan=True, exact_step=True), id="exact")]


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("lossy", LOSS)
@pytest.mark.parametrize("se,traj", [(7, False), (7, True), (1, True)])
def test_two_lanes_per_point_return_the_one_lane_record_on_mirrored_points(se, traj, lossy, check):
    """A sweep's size selects the layout, so two shards of a mirrored sweep must be the whole sweep in every bit: a wave of
    the two-lane kernel whose points all start mirrored takes the one-lane kernel's mirrored z-loop.  A wave of 32 points with
    one asymmetric point, which keeps its wave in the two-lane stage and agrees with the one-lane record to rounding (1e-11,
    the bar between two layouts), then 75 mirrored points: two full waves and a ragged one."""
    rng = np.random.default_rng(75)
    N = 32 + 75
    db, gam, al = rng.uniform(-0.05, 0.05, N), rng.uniform(5e-3, 2e-2, N), rng.uniform(5e-5, 3e-4, N)
    pump = np.sqrt(rng.uniform(0.2, 0.8, N)) * np.exp(1j * rng.uniform(-3.1, 3.1, N))
    side = np.sqrt(rng.uniform(1e-6, 1e-3, N)) * np.exp(1j * rng.uniform(-3.1, 3.1, N))
    a0 = np.column_stack([pump, pump, side, side])
    a0[10, 3] = 1.5 * a0[10, 2]
    mixed, mir = slice(0, 32), slice(32, N)
    kw = dict(n_steps=200, z_max=20.0, save_every=se, **check)
    part = lambda w: dict(gamma=gam[w], alpha=(al[w] if lossy else 0.0), a0=a0[w])   # noqa: E731
    two = nat.sweep_host(db, want_traj=traj, extra_flags=nat.OPT_SPLIT_POINT, **part(slice(0, N)), **kw)
    one = nat.sweep_host(db[mir], want_traj=traj, extra_flags=nat.OPT_ONE_LANE, **part(mir), **kw)
    for k in ("a_end", "p_end", "p_max", "first_bad_step") + (("traj",) if traj else ()):
        assert same_bits(two[k][mir], one[k]), k
    assert (two["first_bad_step"] == -1).all() and np.isfinite(two["a_end"]).all()
    ref = nat.sweep_host(db[mixed], extra_flags=nat.OPT_ONE_LANE, **part(mixed), **kw)
    scale = np.abs(ref["a_end"]).max(axis=1, keepdims=True)
    assert np.max(np.abs(two["a_end"][mixed] - ref["a_end"]) / scale) < 1e-11
    if not traj:
        ws2 = nat.sweep_host(db, wave_summary=True, extra_flags=nat.OPT_SPLIT_POINT, **part(slice(0, N)), **kw)
        ws1 = nat.sweep_host(db[mir], wave_summary=True, extra_flags=nat.OPT_ONE_LANE, **part(mir), **kw)
        for k in ("a_end", "p_end", "p_max", "p_wave_end", "p_wave_max"):
            assert same_bits(ws2[k][mir], ws1[k]), k


def test_failing_mirrored_points_fail_at_the_same_step_in_two_lanes(golden):
    """Golden G9's per-point gamma ladder (first_bad_step [1, 1, 1, 2, 3, 4, 5, -1]) on mirrored points through the two-lane
    launch: the exact index by replay and the block index, as the one-lane kernel reports them."""
    g = golden("G9")
    want = g["first_bad_step"]
    a0 = np.tile(np.sqrt(g["p_in"]).astype(complex), (40, 1))
    assert same_bits(a0[:, 0], a0[:, 1]) and same_bits(a0[:, 2], a0[:, 3])
    gam = np.full(40, g["gammas"][-1])
    gam[0:8] = g["gammas"]
    db = np.full(40, float(g["dbeta"]))
    kw = dict(n_steps=1000, z_max=float(g["z_max"]), save_every=10, gamma=gam, alpha=0.0, a0=a0)
    for exact in (True, False):
        one = nat.sweep_host(db, check_nan=True, exact_step=exact, extra_flags=nat.OPT_ONE_LANE, **kw)
        two = nat.sweep_host(db, check_nan=True, exact_step=exact, extra_flags=nat.OPT_SPLIT_POINT, **kw)
        assert np.array_equal(two["first_bad_step"][0:8], want if exact else np.where(want >= 0, 9, -1))
        assert np.array_equal(two["first_bad_step"], one["first_bad_step"]) and (two["first_bad_step"][8:] == -1).all()
        ok = two["first_bad_step"] == -1
        for k in ("a_end", "p_end", "p_max"):
            assert same_bits(two[k][ok], one[k][ok]), k


def test_the_mirrored_loop_costs_what_its_count_says():
    """The timing recipe of test_gpu_mirrored_waves.py::test_the_mirrored_loop_is_taken -- 65 536 points x 2 000 steps with
    the headline constants on the device API, kernel time from events, median of five launches, mirrored inputs against
    p_in = (0.5, 0.4, 1e-5, 1e-5) -- with the bound of the crosswise step: the midpoint between 1 and 152 / 298."""
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
