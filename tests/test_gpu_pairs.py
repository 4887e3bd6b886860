"""The multi-channel sweep on the GPU (psa_rk4_sweep_pairs_f64: two pumps and K = 1..16 signal/idler pairs, one lane per
pair): ties to the reference's numbers (golden G8) with one pair lit, the existing 6-wave kernel at K = 2, the NumPy
restatement tests/pairs_np.py with every channel lit, the conservation laws, the failure index, save semantics, the device
entry, the device split and the driver.  Shapes are the smallest that can go wrong: 37 points at 16 lanes per point are 592
lanes -- two 256-thread blocks and a ragged wave; K in {3, 5, 11} leave padding lanes."""
import functools

import numpy as np
import pytest

import pairs_np
import psa_amd._native as nat
from conftest import ATOL_DB, RTOL_F64, rel_err
from psa_amd import config, dispersion, scan_mismtach, sweep

pytestmark = pytest.mark.gpu

GAMMA, ALPHA = 0.0115, 1.15e-4
G8_CASES = {"n1e4_a0": ("dbeta257", 0, 10_000), "n1e4_a1": ("dbeta257", 1, 10_000), "n1e5_a1": ("dbeta33", 1, 100_000)}
LIT = sorted({(K, j) for K in (1, 2, 3, 4, 5, 8, 11, 16) for j in (0, K - 1)})


def _waves(K, j):
    return [0, 1, 2 + 2 * j, 3 + 2 * j]


@pytest.mark.parametrize("case", sorted(G8_CASES))
@pytest.mark.parametrize("K,j", LIT)
def test_one_lit_pair_reproduces_the_reference(golden, case, K, j):
    """Only pair j carries light; the dark pairs have random mismatches.  The lit columns and the pumps are golden G8 (the
    reference's own runs, 1e5 steps on dbeta33 included), the dark columns exactly 0."""
    g = golden("G8")
    key, ia, n = G8_CASES[case]
    db = g[key]
    N = db.size
    rng = np.random.default_rng(100 * K + j)
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    dbeta[:, j] = db
    a0 = np.zeros(2 + 2 * K, complex)
    a0[_waves(K, j)] = np.sqrt(g["p_in"])
    r = nat.sweep_pairs_host(dbeta, n_steps=n, z_max=float(g["z_max"]), save_every=int(g["save_every"]), gamma=float(g["gamma"]),
                             alpha=float(g["alphas"][ia]), a0=a0)
    w = _waves(K, j)
    err_a = rel_err(r["a_end"][:, w], g[case + "_A_end"])
    err_e = rel_err(r["p_wave_end"][:, w[2]], g[case + "_p_end"])
    err_m = rel_err(r["p_wave_max"][:, w[2]], g[case + "_p_max"])
    print(f"K={K} j={j} {case}: a_end {err_a:.2e} p_end {err_e:.2e} p_max {err_m:.2e}")
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64
    dark = [c for c in range(2 + 2 * K) if c not in w]
    assert np.all(r["a_end"][:, dark] == 0) and np.all(r["p_wave_end"][:, dark] == 0) and np.all(r["p_wave_max"][:, dark] == 0)
    assert (r["first_bad_step"] == -1).all()


def test_two_pairs_equal_the_six_wave_kernel():
    """K = 2 is the 6-wave model: against rk4_sweep_kernel with one lane per point on the 203 random points of
    test_exchanging_the_pairs_permutes_the_output, 1 500 steps, within 1e-11 of the point's largest wave -- the project's
    bar for two layouts of one model."""
    rng = np.random.default_rng(11)
    N = 203
    db1, db2 = rng.uniform(-0.05, 0.05, N), rng.uniform(-0.05, 0.05, N)
    p = np.column_stack([rng.uniform(0.2, 0.6, (N, 2)), 10 ** rng.uniform(-6, -3, (N, 4))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 6)))
    kw = dict(n_steps=1500, z_max=150.0, save_every=10, gamma=GAMMA, alpha=ALPHA, a0=a0)
    six = nat.sweep_host(db1, dbeta2=db2, extra_flags=nat.OPT_ONE_LANE, wave_summary=True, **kw)
    got = nat.sweep_pairs_host(np.column_stack([db1, db2]), **kw)
    scale = np.abs(six["a_end"]).max(axis=1, keepdims=True)
    err = np.max(np.abs(got["a_end"] - six["a_end"]) / scale)
    print(f"K=2 vs 6-wave one-lane: {err:.2e}")
    assert err < 1e-11
    assert rel_err(got["p_wave_end"], six["p_wave_end"]) < 1e-10 and rel_err(got["p_wave_max"], six["p_wave_max"]) < 1e-10
    assert np.array_equal(got["first_bad_step"], six["first_bad_step"])


@functools.lru_cache(maxsize=None)
def _all_lit(K, per_point):
    """Inputs and the restatement's answer, computed once per case: G8's fibre and powers on every channel."""
    N, n, z_max = 37, 10_000, 1000.0
    rng = np.random.default_rng(7 * K + per_point)
    dbeta = np.linspace(-0.05, 0.05, N)[:, None] * np.linspace(1.0, 0.5, K)[None, :]
    p = np.empty(2 + 2 * K)
    p[:2], p[2:] = 0.5, 1e-5
    if per_point:
        a0 = np.sqrt(p)[None, :] * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))
        gamma, alpha = GAMMA * rng.uniform(0.9, 1.1, N), ALPHA * rng.uniform(0.5, 1.5, N)
    else:
        a0, gamma, alpha = np.sqrt(p).astype(complex), GAMMA, ALPHA
    ref = pairs_np.integrate(a0, dbeta, z_max=z_max, n=n, save_every=10, gamma=gamma, alpha=alpha)
    return dict(dbeta=dbeta, a0=a0, gamma=gamma, alpha=alpha, n=n, z_max=z_max, ref=ref)


@pytest.mark.parametrize("per_point", [True, False], ids=["per_point", "broadcast"])
@pytest.mark.parametrize("K", [3, 8, 16])
def test_all_channels_lit_match_the_restatement_and_conserve(K, per_point):
    """Every channel lit: a_end within RTOL_F64 of the point's largest wave, the power summary within RTOL_F64, and on every
    point total power * e^{alpha L}, each pair's |s|^2 - |i|^2 and |p1|^2 - |p2|^2 (the Manley-Rowe differences, likewise
    scaled) within 1e-9 of the input total (the NumPy probe holds them to better than 1e-12 W)."""
    c = _all_lit(K, per_point)
    r = nat.sweep_pairs_host(c["dbeta"], n_steps=c["n"], z_max=c["z_max"], save_every=10, gamma=c["gamma"], alpha=c["alpha"],
                             a0=c["a0"])
    ref = c["ref"]
    scale = np.abs(ref["a_end"]).max(axis=1, keepdims=True)
    err_a = np.max(np.abs(r["a_end"] - ref["a_end"]) / scale)
    err_e, err_m = rel_err(r["p_wave_end"], ref["p_wave_end"]), rel_err(r["p_wave_max"], ref["p_wave_max"])
    print(f"K={K} per_point={per_point}: a_end {err_a:.2e} p_wave_end {err_e:.2e} p_wave_max {err_m:.2e}")
    assert (r["first_bad_step"] == -1).all() and (ref["first_bad_step"] == -1).all()
    assert err_a < RTOL_F64 and err_e < RTOL_F64 and err_m < RTOL_F64
    p_in = np.broadcast_to(np.abs(np.atleast_2d(c["a0"])) ** 2, r["p_wave_end"].shape)
    p_out = r["p_wave_end"] * np.exp(np.broadcast_to(c["alpha"], (37,)) * c["z_max"])[:, None]
    total = p_in.sum(axis=1)
    d_total = np.abs(p_out.sum(axis=1) - total) / total
    d_pumps = np.abs((p_out[:, 0] - p_out[:, 1]) - (p_in[:, 0] - p_in[:, 1])) / total
    d_pairs = np.abs((p_out[:, 2::2] - p_out[:, 3::2]) - (p_in[:, 2::2] - p_in[:, 3::2])) / total[:, None]
    print(f"   conservation: total {d_total.max():.2e} pumps {d_pumps.max():.2e} pairs {d_pairs.max():.2e}")
    assert d_total.max() < 1e-9 and d_pumps.max() < 1e-9 and d_pairs.max() < 1e-9


@pytest.mark.parametrize("K", [5, 16])
def test_permuting_the_pairs_permutes_the_output(K):
    """Pairs and their dbeta columns permuted together: the output permutes -- to ROUNDING (1e-11 of the point's largest
    wave after 1 500 steps), not bit for bit: the butterfly adds the pair terms in an order fixed by the lane numbers, so a
    permutation changes the order of the additions behind the pumps' sums, as exchanging the pairs does in the 6-wave
    kernels."""
    rng = np.random.default_rng(K)
    N = 37
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    p = np.column_stack([rng.uniform(0.2, 0.6, (N, 2)), 10 ** rng.uniform(-6, -3, (N, 2 * K))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))
    perm = rng.permutation(K)
    cols = np.concatenate([[0, 1], np.column_stack([2 + 2 * perm, 3 + 2 * perm]).ravel()])
    kw = dict(n_steps=1500, z_max=150.0, save_every=10, gamma=GAMMA, alpha=ALPHA)
    a = nat.sweep_pairs_host(dbeta, a0=a0, **kw)
    b = nat.sweep_pairs_host(dbeta[:, perm], a0=a0[:, cols], **kw)
    scale = np.abs(a["a_end"]).max(axis=1, keepdims=True)
    err = np.max(np.abs(a["a_end"][:, cols] - b["a_end"]) / scale)
    print(f"K={K}: permuted output differs by {err:.2e}")
    assert err < 1e-11
    assert rel_err(b["p_wave_max"], a["p_wave_max"][:, cols]) < 1e-10
    assert np.array_equal(a["first_bad_step"], b["first_bad_step"])


def _failing_inputs():
    K, N = 5, 9
    a0 = np.zeros(2 + 2 * K, complex)
    a0[:2], a0[2::2] = np.sqrt(0.5), np.sqrt(1e-5)
    dbeta = np.linspace(-0.05, 0.05, N)[:, None] * np.linspace(1.0, 0.5, K)
    return dbeta, dict(n_steps=2000, z_max=200.0, save_every=10, gamma=GAMMA, alpha=-np.linspace(3.2, 12, N), a0=a0)


def test_failure_index_exact_block_and_unchecked():
    """A gain of 3.2 .. 12 per metre overflows within 25 steps.  The exact index is the restatement's (computed on the CPU;
    unchanged under a 1e-9 perturbation of alpha); block mode reports the last step of the first non-finite save block;
    without check_nan the index is -1 and the outputs are NaN."""
    want = np.array([23, 18, 15, 12, 11, 9, 9, 8, 7])
    dbeta, kw = _failing_inputs()
    ref = pairs_np.integrate(kw["a0"], dbeta, z_max=200.0, n=2000, save_every=10, gamma=GAMMA, alpha=kw["alpha"])
    assert np.array_equal(ref["first_bad_step"], want)
    exact =nat.sweep_pairs_host(dbeta, exact_step=True, **kw)
    print("exact", exact["first_bad_step"])
    assert np.array_equal(exact["first_bad_step"], want)
    block = nat.sweep_pairs_host(dbeta, exact_step=False, **kw)
    print("block", block["first_bad_step"])
    assert np.array_equal(block["first_bad_step"], want // 10 * 10 + 9)
    off = nat.sweep_pairs_host(dbeta, check_nan=False, **kw)
    assert (off["first_bad_step"] == -1).all()
    assert np.isnan(off["a_end"]).all() and np.isnan(off["p_wave_end"]).all() and np.isnan(off["p_wave_max"]).all()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "block"])
def test_a_failing_point_leaves_its_wave_neighbours_untouched(exact):
    """One failing point among 36 healthy ones at K = 3: it shares a wave (16 points of 4 lanes) with others, and the replay
    it triggers runs in their lanes too.  Their outputs equal the run without the failure bit for bit."""
    N, K = 37, 3
    rng = np.random.default_rng(3)
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    p = np.column_stack([np.full((N, 2), 0.5), 10 ** rng.uniform(-6, -4, (N, 2 * K))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))
    alpha = np.full(N, ALPHA)
    kw = dict(n_steps=1005, z_max=100.5, save_every=10, gamma=GAMMA, a0=a0, exact_step=exact)
    clean = nat.sweep_pairs_host(dbeta, alpha=alpha, **kw)
    alpha_bad = alpha.copy()
    alpha_bad[17] = -8.0
    bad = nat.sweep_pairs_host(dbeta, alpha=alpha_bad, **kw)
    ok = np.arange(N) != 17
    assert (clean["first_bad_step"] == -1).all()
    assert bad["first_bad_step"][17] >= 0 and (bad["first_bad_step"][ok] == -1).all()
    ref = pairs_np.integrate(a0[17], dbeta[17:18], z_max=100.5, n=1005, save_every=10, gamma=GAMMA, alpha=-8.0)
    want = int(ref["first_bad_step"][0])
    assert bad["first_bad_step"][17] == (want if exact else want // 10 * 10 + 9)
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(bad[key][ok], clean[key][ok]), key


def test_save_semantics():
    """n_steps = 1005 with save_every = 10: a_end is the state after step 1000 and the maxima run over the saved rows
    including z = 0; save_every > n_steps: the only row is z = 0, so a_end is a0."""
    N, K = 5, 3
    rng = np.random.default_rng(5)
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    p = np.column_stack([np.full((N, 2), 0.5), 10 ** rng.uniform(-6, -4, (N, 2 * K))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))
    kw = dict(z_max=100.5, gamma=GAMMA, alpha=ALPHA)
    r = nat.sweep_pairs_host(dbeta, n_steps=1005, save_every=10, a0=a0, **kw)
    ref = pairs_np.integrate(a0, dbeta, n=1005, save_every=10, **kw)
    tail = pairs_np.integrate(a0, dbeta, n=1005, save_every=1005, **kw)      # the state after all 1005 steps: another one
    assert rel_err(r["a_end"], ref["a_end"]) < RTOL_F64 and rel_err(ref["a_end"], tail["a_end"]) > 1e-6
    assert rel_err(r["p_wave_end"], ref["p_wave_end"]) < RTOL_F64 and rel_err(r["p_wave_max"], ref["p_wave_max"]) < RTOL_F64
    assert np.all(r["p_wave_max"][:, :2] >= p[:, :2] * (1 - 1e-15))          # z = 0 is a saved row: the pumps only deplete
    r0 = nat.sweep_pairs_host(dbeta, n_steps=7, save_every=10, a0=a0, **kw)
    assert np.array_equal(r0["a_end"], a0) and (r0["first_bad_step"] == -1).all()
    assert rel_err(r0["p_wave_end"], p) < 1e-15 and np.array_equal(r0["p_wave_end"], r0["p_wave_max"])


@pytest.mark.parametrize("K", [3, 16])
def test_the_stride_does_not_change_the_computed_rows(K):
    """The re-seeds sit on the absolute step grid, so the last saved row at stride se is the state after m = 200 // se * se
    steps whatever se is: it equals, bit for bit, the end of a run of m steps saved once (h = 0.5 m is exact in both) --
    below, at and above RESYNC = 64; the run saved once re-seeds inside its only block.  se > n_steps: the only row is
    z = 0."""
    N = 37
    rng = np.random.default_rng(40 + K)
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    p = np.column_stack([np.full((N, 2), 0.5), 10 ** rng.uniform(-6, -4, (N, 2 * K))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 2 + 2 * K)))
    kw = dict(gamma=GAMMA, alpha=ALPHA, a0=a0)
    for se in (7, 64, 65):
        m = 200 // se * se
        r = nat.sweep_pairs_host(dbeta, n_steps=200, z_max=100.0, save_every=se, **kw)
        once = nat.sweep_pairs_host(dbeta, n_steps=m, z_max=0.5 * m, save_every=m, **kw)
        assert (r["first_bad_step"] == -1).all() and np.isfinite(r["a_end"].view(float)).all()
        assert np.array_equal(r["a_end"], once["a_end"]), se
        assert np.array_equal(r["p_wave_end"], once["p_wave_end"]), se
    r = nat.sweep_pairs_host(dbeta, n_steps=200, z_max=100.0, save_every=1000, **kw)
    assert np.array_equal(r["a_end"], a0) and (r["first_bad_step"] == -1).all()


@functools.lru_cache(maxsize=None)
def _graded_failures():
    """The inputs of test_gpu_lanes' replay test at K = 3: 60 of 331 points get a graded gain and blow up at step indices
    spread over the run.  With them the block-mode run at save_every = 1: a block is a step there, so its index is the
    per-step index and no replay is involved."""
    n, N = 450, 331
    rng = np.random.default_rng(7)
    db = rng.uniform(-0.05, 0.05, N)
    al = np.full(N, ALPHA)
    hot = rng.choice(N, 60, replace=False)
    al[hot] = -np.geomspace(1.0, 60.0, hot.size)
    a0 = np.zeros(8, complex)
    a0[:2], a0[2:] = np.sqrt(0.5), np.sqrt(1e-5)
    dbeta = db[:, None] * np.linspace(1.0, 0.5, 3)
    kw = dict(n_steps=n, z_max=45.0, gamma=GAMMA, alpha=al, a0=a0)
    per_step = nat.sweep_pairs_host(dbeta, save_every=1, exact_step=False, **kw)["first_bad_step"]
    return dbeta, kw, per_step


@pytest.mark.parametrize("se", [7, 64, 1024])
def test_exact_index_equals_the_per_step_index(se):
    """The replay of a failing block repeats the forward pass, so the index it finds is the one a test after every step finds
    -- inside saved blocks, across the 64-step re-seeds and (se = 1024) in a run without a saved row.  Block mode names the
    block of that index, and finite points are bit-identical in both modes."""
    n = 450
    dbeta, kw, per_step = _graded_failures()
    failed = per_step >= 0
    print(f"failing points {failed.sum()}, distinct indices {len(set(per_step[failed]))}, largest {per_step.max()}")
    assert failed.sum() >= 40 and len(set(per_step[failed])) >= 20 and per_step.max() >= 100
    got = nat.sweep_pairs_host(dbeta, save_every=se, exact_step=True, **kw)
    blk = nat.sweep_pairs_host(dbeta, save_every=se, exact_step=False, **kw)
    assert np.array_equal(got["first_bad_step"], per_step)
    exact, last_saved = per_step[failed], n // se * se
    assert np.array_equal(blk["first_bad_step"][failed], np.where(exact // se * se + se <= last_saved, exact // se * se + se - 1, n - 1))
    assert (blk["first_bad_step"][~failed] == -1).all()
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(got[key][~failed], blk[key][~failed]), key


def test_device_entry_and_device_split_equal_the_host_entry_bit_for_bit():
    torch = pytest.importorskip("torch")
    N, K = 37, 11
    nw = 2 + 2 * K
    rng = np.random.default_rng(9)
    dbeta = rng.uniform(-0.05, 0.05, (N, K))
    p = np.column_stack([np.full((N, 2), 0.5), 10 ** rng.uniform(-6, -4, (N, 2 * K))])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, nw)))
    gamma = GAMMA * rng.uniform(0.9, 1.1, N)
    kw = dict(z_max=100.0, n_steps=1000, save_every=10, gamma=gamma, alpha=ALPHA, a0=a0)
    host = sweep.rk4_sweep_pairs(dbeta, **kw)
    split = sweep.rk4_sweep_pairs(dbeta, devices=[0, 0], **kw)
    for key in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step"):
        assert np.array_equal(getattr(host, key), getattr(split, key)), key

    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_db, d_g, d_al = t(dbeta.T), t(gamma), t(np.array([ALPHA]))
    d_a0 = t(a0.view(np.float64).reshape(N, 2 * nw).T)
    d_aend = torch.empty((2 * nw, N), dtype=torch.float64, device=dev)
    d_we, d_wm = torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    nat.sweep_pairs_device(stream=torch.cuda.current_stream().cuda_stream, n_pairs=K, n_points=N, n_steps=1000, z_max=100.0,
                           save_every=10, d_dbeta_soa=d_db.data_ptr(), d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(),
                           d_a0_soa=d_a0.data_ptr(), flags=nat.BCAST_ALPHA | nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP,
                           d_a_end_soa=d_aend.data_ptr(), d_p_wave_end_soa=d_we.data_ptr(),
                           d_p_wave_max_soa=d_wm.data_ptr(), d_first_bad=d_bad.data_ptr())
    torch.cuda.synchronize()
    a_end = np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128)
    assert np.array_equal(a_end, host.a_end)
    assert np.array_equal(d_we.cpu().numpy().T, host.p_wave_end) and np.array_equal(d_wm.cpu().numpy().T, host.p_wave_max)
    assert np.array_equal(d_bad.cpu().numpy(), host.first_bad_step)


def test_wdm_driver(golden):
    """scan_wdm_gain with one channel is the 4-wave sweep at the same dbeta (within ATOL_DB); with eight channels it is a
    direct rk4_sweep_pairs call on the mismatches it reports."""
    dv = golden("G11")["disp_m"]
    d = dispersion.DispersionParams(omega_ref=dv[0], beta2=dv[1], beta3=dv[2], beta4=dv[3])
    cfg = config.custom_simulation_config(z_max=300.0, dz=0.1)
    common = dict(cfg=cfg, lambda_p1_m=1550e-9, lambda_p2_m=1556e-9, p_pump=[0.3, 0.25], gamma=GAMMA, alpha=1.0e-4,
                  dispersion=d)
    ps1 = np.array([[2e-6], [5e-6], [1e-5]])
    one = scan_mismtach.scan_wdm_gain(Omega=[4e12], p_signal=ps1, p_idler=5e-7, **common)
    assert one["gain"].shape == (3, 1) and one["idler"].shape == (3, 1) and one["pump_depletion"].shape == (3,)
    for k in range(3):
        a0 = np.sqrt(np.array([0.3, 0.25, ps1[k, 0], 5e-7])).astype(complex)
        ref = sweep.rk4_sweep(one["dbeta"], z_max=300.0, n_steps=3000, save_every=cfg.save_every, gamma=GAMMA, alpha=1.0e-4,
                              a0=a0)
        assert abs(one["gain"][k, 0] - ref.gain(ps1[k, 0])[0]) < ATOL_DB
    Om = np.linspace(2e12, 9e12, 8)
    ps8 = np.outer([1.0, 10.0, 100.0], np.full(8, 1e-6))
    out = scan_mismtach.scan_wdm_gain(Omega=Om, p_signal=ps8, **common)
    p_all = np.zeros((3, 18))
    p_all[:, 0], p_all[:, 1], p_all[:, 2::2] = 0.3, 0.25, ps8
    direct = sweep.rk4_sweep_pairs(np.broadcast_to(out["dbeta"], (3, 8)), z_max=300.0, n_steps=3000, save_every=cfg.save_every,
                                   gamma=GAMMA, alpha=1.0e-4, a0=np.sqrt(p_all).astype(complex))
    assert np.array_equal(out["result"].a_end, direct.a_end) and (out["first_bad_step"] == -1).all()
    assert np.array_equal(out["gain"], direct.channel_gain(ps8)) and np.array_equal(out["idler"], direct.idler_conversion(ps8))
    assert np.array_equal(out["pump_depletion"], direct.pump_depletion())
