"""Multi-channel fibre chains and saved rows on the GPU (psa_rk4_pairs_chain_f64, sweep.rk4_chain_pairs,
rk4_sweep_pairs(want_traj=True), scan_mismtach.scan_wdm_copier_psa_phase) against the NumPy restatement
tests/pairs_chain_np.py at the project's bar RTOL_F64 (1e-9 of the point's largest wave):

* the rows of one span for K = 1, 3, 16 (L = 2, 4, 16 lanes per point; 70 points with K = 3 are 280 lanes: more than one
  256-thread block, no multiple of 64), every step and every 7th of 130 saved; the summaries with and without rows bit-equal;
* one span without rows is psa_rk4_sweep_pairs_f64 bit for bit;
* K = 1 against rk4_chain on 4 waves and K = 2 against rk4_chain on 6 waves at 1e-10;
* one fibre cut into 2, 3 and 7 spans with identity transfers is the unsplit sweep;
* a lossy three-span chain with per-point dbeta (N, K), gamma, alpha, a per-point and a broadcast transfer: 300 points cross
  a 256-thread epilogue block;
* spans of 1, 63, 64, 65 and 130 steps in one chain (the kernel re-seeds its phase every 64 steps);
* permuting the pairs permutes the outputs;
* a failure in span 2 is reported at the chain's step index, exact and per save block, its neighbours untouched;
* the `_dev` entry on a caller's workspace of exactly the stated size and padded trajectory rows, bit-equal to the host form;
* devices=[0, 0] equals one device; the phase-scan driver against the dual-pump closed form and a direct chain call."""
import functools

import numpy as np
import pytest

import pairs_chain_np as chain_np
import psa_amd._native as nat
from conftest import RTOL_F64
from psa_amd import config, dispersion, scan_mismtach
from psa_amd.sweep import FibreSpan, rk4_chain, rk4_chain_pairs, rk4_sweep_pairs

pytestmark = pytest.mark.gpu

KEYS = ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")


def wave_err(got, ref):
    """max |got - ref| over the largest wave of the point (amplitudes (N, ..., NW) complex)."""
    ref = np.asarray(ref)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return float(np.max(np.abs(np.asarray(got) - ref) / scale))


def power_err(got, ref):
    """The same bar on a power summary (N, NW): the waves' moduli sqrt(P_j) against the point's largest."""
    return wave_err(np.sqrt(np.asarray(got)).astype(complex), np.sqrt(np.asarray(ref)).astype(complex))


def _fibre(spans):
    return [FibreSpan(L, n_steps=n, dbeta=db, gamma=g, alpha=al) for L, n, db, g, al in spans]


def _strided(rows, z_out, steps, se):
    """Rows of a chain saved every ``se`` steps, out of the rows saved at every step."""
    offs = np.concatenate([[0], np.cumsum(np.asarray(steps) + 1)[:-1]])
    idx = np.concatenate([o + np.arange(0, s - s % se + 1, se) for o, s in zip(offs, steps)])
    return rows[:, idx], z_out[idx]


# ---- rows of one span -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_span(K):
    """70 points, 130 steps, every step saved by the restatement; any stride is read off its rows."""
    rng = np.random.default_rng(100 + K)
    N = 70
    a0 = chain_np.random_a0(rng, N, K)
    db = rng.uniform(-3.5, 1.5, (N, K)) * chain_np.GAMMA * 2 * chain_np.P_PUMP
    gamma, alpha = chain_np.GAMMA * rng.uniform(0.8, 1.6, N), 1.15e-4 * rng.uniform(0.5, 2.0, N)
    ref = chain_np.integrate(a0, db, z_max=260.0, n=130, save_every=1, gamma=gamma, alpha=alpha)
    assert (ref["first_bad_step"] == -1).all()
    return a0, db, gamma, alpha, ref["traj"]


@pytest.mark.parametrize("save_every", [1, 7])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_rows_of_one_span_against_the_restatement(K, save_every):
    a0, db, gamma, alpha, rows = _one_span(K)
    want = rows[:, ::save_every]
    kw = dict(z_max=260.0, n_steps=130, save_every=save_every, gamma=gamma, alpha=alpha, a0=a0)
    got = rk4_sweep_pairs(db, want_traj=True, **kw)
    assert got.traj.shape == want.shape == (70, 130 // save_every + 1, 2 + 2 * K)
    errs = (wave_err(got.traj, want), wave_err(got.a_end, want[:, -1]), power_err(got.p_wave_end, np.abs(want[:, -1]) ** 2),
            power_err(got.p_wave_max, np.max(np.abs(want) ** 2, axis=1)))
    print(f"K = {K}, save_every = {save_every}: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} "
          f"p_wave_max {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    assert np.array_equal(got.traj[:, 0], a0) and np.array_equal(got.traj[:, -1], got.a_end)
    lean = rk4_sweep_pairs(db, **kw)
    assert lean.traj is None
    for key in KEYS:
        assert np.array_equal(getattr(lean, key), getattr(got, key)), key


@pytest.mark.parametrize("K", [1, 3, 16])
def test_one_span_without_rows_is_the_sweep_bit_for_bit(K):
    a0, db, gamma, alpha, _ = _one_span(K)
    kw = dict(save_every=10, a0=a0)
    ref = nat.sweep_pairs_host(db, n_steps=130, z_max=260.0, gamma=gamma, alpha=1.15e-4, **kw)
    got = nat.pairs_chain_host(db[None], n_steps=[130], seg_len=[260.0], gamma=gamma[None], alpha=[1.15e-4], **kw)
    for key in KEYS:
        assert np.array_equal(got[key], ref[key], equal_nan=True), key
    assert got["traj"] is None and got["first_bad_step"].shape == (70,)


# ---- K = 1 and K = 2 are the 4- and the 6-wave chain ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2])
def test_one_and_two_pairs_against_rk4_chain(K):
    """Three lossy spans with per-point transfers (the broadcast one tiled); the kernels order the triple products differently,
    so they agree to rounding: 1e-10 of the point's largest wave on inputs that tests/test_pairs_chain_host.py shows to be
    well conditioned (a 1e-14 perturbation moves the rows by less than 1e-12)."""
    a0, spans, transfers = chain_np.lossy_case(70, K, seed=21, steps=(60, 100, 40))
    transfers = [np.broadcast_to(t, a0.shape) for t in transfers]
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    got = rk4_chain_pairs(_fibre(spans), **kw)
    other = [FibreSpan(L, n_steps=n, dbeta=db[:, 0], dbeta2=(db[:, 1] if K == 2 else None), gamma=g, alpha=al)
             for L, n, db, g, al in spans]
    ref = rk4_chain(other, **kw)
    waves = rk4_chain(other, **dict(kw, want_traj=False, wave_summary=True))   # the per-wave summary takes no trajectory
    errs = (wave_err(got.traj, ref.traj), wave_err(got.a_end, ref.a_end), power_err(got.p_wave_end, waves.p_wave_end),
            power_err(got.p_wave_max, waves.p_wave_max))
    print(f"K = {K} against rk4_chain on {2 + 2 * K} waves: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} "
          f"p_wave_max {errs[3]:.2e}")
    assert got.traj.shape == ref.traj.shape == (70, 4 + 6 + 3, 2 + 2 * K) and max(errs) < 1e-10
    assert np.array_equal(got.first_bad_step, ref.first_bad_step) and np.array_equal(got.z_out, ref.z_out)


# ---- identity split -------------------------------------------------------------------------------------------------------
def _split(n, cuts, se):
    steps = np.full(cuts, (n // se // cuts) * se)
    steps[-1] = n - steps[:-1].sum()
    return [int(s) for s in steps]


def _rows(steps, se):
    offs = np.concatenate([[0], np.cumsum(steps)[:-1]])
    return np.concatenate([o // se + np.arange(s // se + 1) for o, s in zip(offs, steps)])


@functools.lru_cache(maxsize=None)
def _unsplit():
    n_pts, K, n, L, se = 33, 5, 1400, 700.0, 10
    rng = np.random.default_rng(2)
    a0 = chain_np.random_a0(rng, n_pts, K)
    db = rng.uniform(-3.5, 1.5, (n_pts, K)) * chain_np.GAMMA * 2 * chain_np.P_PUMP
    gamma, alpha = chain_np.GAMMA * rng.uniform(0.9, 1.1, n_pts), 1.15e-4 * rng.uniform(0.5, 1.5, n_pts)
    whole = rk4_sweep_pairs(db, z_max=L, n_steps=n, save_every=se, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    return db, a0, gamma, alpha, whole


@pytest.mark.parametrize("cuts", [2, 3, 7])
def test_identity_split_equals_the_unsplit_run(cuts):
    n_pts, K, n, L, se = 33, 5, 1400, 700.0, 10
    db, a0, gamma, alpha, whole = _unsplit()
    steps = _split(n, cuts, se)
    spans = [FibreSpan(L * s / n, n_steps=s, dbeta=db, gamma=gamma, alpha=alpha) for s in steps]
    got = rk4_chain_pairs(spans, a0=a0, transfers=[np.ones(2 + 2 * K)] * (cuts - 1), save_every=se, want_traj=True)
    assert got.traj.shape == (n_pts, sum(s // se + 1 for s in steps), 2 + 2 * K) and got.n_steps == n
    np.testing.assert_allclose(got.z_out, np.linspace(0, L, n + 1)[::se][_rows(steps, se)], rtol=1e-12, atol=1e-9)
    errs = dict(a_end=wave_err(got.a_end, whole.a_end), p_wave_end=power_err(got.p_wave_end, whole.p_wave_end),
                p_wave_max=power_err(got.p_wave_max, whole.p_wave_max), rows=wave_err(got.traj, whole.traj[:, _rows(steps, se)]))
    print(f"{cuts} spans against the unsplit sweep: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL_F64
    assert np.all(got.first_bad_step == -1)
    # without the trajectory the summaries are the same numbers
    lean = rk4_chain_pairs(spans, a0=a0, save_every=se)
    for key in KEYS:
        assert np.array_equal(getattr(lean, key), getattr(got, key)), key
    assert lean.traj is None


# ---- the lossy three-span chain -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lossy_reference(K):
    """300 points through the restatement once, every step saved; any save stride is read off the rows."""
    case = chain_np.lossy_case(300, K, steps=(120, 200, 80))
    ref = chain_np.chain(*case, 1)
    assert (ref["first_bad_step"] == -1).all()
    return case, ref["rows"], ref["z_out"]


@pytest.mark.parametrize("save_every", [1, 20])
@pytest.mark.parametrize("K", [3, 16])
def test_lossy_chain_with_transfers_against_the_restatement(K, save_every):
    (a0, spans, transfers), rows, z_all = _lossy_reference(K)
    want, z_want = _strided(rows, z_all, [n for _, n, *_ in spans], save_every)
    got = rk4_chain_pairs(_fibre(spans), a0=a0, transfers=transfers, save_every=save_every, want_traj=True)
    assert got.traj.shape == want.shape
    errs = (wave_err(got.traj, want), wave_err(got.a_end, want[:, -1]), power_err(got.p_wave_end, np.abs(want[:, -1]) ** 2),
            power_err(got.p_wave_max, np.max(np.abs(want) ** 2, axis=1)))
    print(f"lossy 3-span chain, K = {K}, 300 points, save_every={save_every}: rows {errs[0]:.2e} a_end {errs[1]:.2e} "
          f"p_wave_end {errs[2]:.2e} p_wave_max {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    np.testing.assert_allclose(got.z_out, z_want, rtol=1e-14, atol=0.0)
    assert np.all(got.first_bad_step == -1) and np.array_equal(got.traj[:, -1], got.a_end)
    assert np.array_equal(got.row_offsets, np.concatenate([[0], np.cumsum([n // save_every + 1 for _, n, *_ in spans])]))


def test_loop_edges_in_one_chain():
    """Spans of 1, 63, 64, 65 and 130 steps, every step saved, per-point transfers between them."""
    N, K, steps = 70, 3, (1, 63, 64, 65, 130)
    rng = np.random.default_rng(5)
    a0 = chain_np.random_a0(rng, N, K)
    G, P = chain_np.GAMMA, 2 * chain_np.P_PUMP
    spans = [(2.0 * n, n, rng.uniform(-3.5, 1.5, (N, K)) * G * P, G * rng.uniform(0.9, 1.3, N), 1.15e-4 * rng.uniform(0.0, 2.0, N))
             for n in steps]
    transfers = [chain_np.mid_stage(rng.uniform(-2, 1, (N, 8)), rng.uniform(-np.pi, np.pi, (N, 8))) for _ in steps[1:]]
    ref = chain_np.chain(a0, spans, transfers, 1)
    got = rk4_chain_pairs(_fibre(spans), a0=a0, transfers=transfers, save_every=1, want_traj=True)
    errs = (wave_err(got.traj, ref["rows"]), wave_err(got.a_end, ref["a_end"]), power_err(got.p_wave_max, ref["p_wave_max"]))
    print(f"loop edges: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_max {errs[2]:.2e}")
    assert got.traj.shape == (N, sum(steps) + len(steps), 8) and max(errs) < RTOL_F64 and np.all(got.first_bad_step == -1)


def test_permuting_the_pairs_permutes_the_outputs():
    """K = 5 (three padding lanes), two spans: pair k moved to lane perm[k].  The sums over the pairs are formed in another
    order, so the outputs agree to rounding (RTOL_F64), not bit for bit."""
    N, K = 40, 5
    a0, spans, transfers = chain_np.lossy_case(N, K, seed=9, steps=(100, 60), lengths=(250.0, 150.0))
    transfers = transfers[:1]
    perm = np.array([3, 0, 4, 2, 1])
    wave = np.concatenate([[0, 1], np.stack([2 + 2 * perm, 3 + 2 * perm], axis=1).ravel()])
    kw = dict(save_every=20, want_traj=True)
    base = rk4_chain_pairs(_fibre(spans), a0=a0, transfers=transfers, **kw)
    moved = rk4_chain_pairs(_fibre([(L, n, db[:, perm], g, al) for L, n, db, g, al in spans]), a0=a0[:, wave],
                            transfers=[t[:, wave] for t in transfers], **kw)
    errs = (wave_err(moved.traj, base.traj[:, :, wave]), wave_err(moved.a_end, base.a_end[:, wave]),
            power_err(moved.p_wave_max, base.p_wave_max[:, wave]), power_err(moved.p_wave_end, base.p_wave_end[:, wave]))
    print(f"permuted pairs: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_max {errs[2]:.2e} p_wave_end {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    ref = chain_np.chain(a0, spans, transfers, 20)
    assert wave_err(base.traj, ref["rows"]) < RTOL_F64


def test_first_bad_step_of_a_failure_in_span_two_is_cumulative():
    """Span 2 is past the RK4 stability edge at points 1 and 3 (gamma 300): the restatement fails there at local step 1
    (tests/test_pairs_chain_host.py), so the chain reports 400 + 1 exactly and 400 + 9, the last step of the save block,
    without exact_step.  The five points share one 64-lane wave (4 lanes each): the healthy ones are untouched."""
    a0, spans = chain_np.failing_case()
    ref = chain_np.chain(a0, spans, [np.ones(8)], 10)
    assert np.array_equal(ref["first_bad_step"], [-1, 401, -1, 401, -1])
    kw = dict(a0=a0, transfers=[np.ones(8)], save_every=10)
    got = rk4_chain_pairs(_fibre(spans), exact_step=True, **kw)
    block = rk4_chain_pairs(_fibre(spans), exact_step=False, **kw)
    np.testing.assert_array_equal(got.first_bad_step, [-1, 401, -1, 401, -1])
    np.testing.assert_array_equal(block.first_bad_step, [-1, 409, -1, 409, -1])
    ok = [0, 2, 4]
    for r in (got, block):
        assert np.all(np.isnan(r.p_wave_max[[1, 3]])) and np.all(np.isfinite(r.p_wave_max[ok]))
        g = r.channel_gain(np.full(3, 1e-5), mode="max")
        assert np.all(np.isnan(g[[1, 3]])) and np.all(np.isfinite(g[ok]))
        errs = (wave_err(r.a_end[ok], ref["a_end"][ok]), power_err(r.p_wave_end[ok], ref["p_wave_end"][ok]),
                power_err(r.p_wave_max[ok], ref["p_wave_max"][ok]))
        assert max(errs) < RTOL_F64
    for key in ("a_end", "p_wave_end", "p_wave_max"):
        assert np.array_equal(getattr(got, key)[ok], getattr(block, key)[ok]), key


# ---- the _dev entry -------------------------------------------------------------------------------------------------------
def _device_chain(torch, a0, spans, transfers, *, save_every, flags, ld):
    """psa_rk4_pairs_chain_f64_dev on torch buffers with a workspace of exactly the stated size (and a guard behind it) -> the
    host entry's dictionary, the trajectory's padding and the guard."""
    dev = torch.device("cuda:0")
    N, nw, S = a0.shape[0], a0.shape[1], len(spans)
    K = (nw - 2) // 2
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_db = t(np.stack([sp[2] for sp in spans]).transpose(0, 2, 1))                       # (S, K, N)
    d_g, d_al = (t(np.stack([sp[k] for sp in spans])) for k in (3, 4))
    d_a0 = t(a0.view(np.float64).reshape(N, 2 * nw).T)
    tr = np.stack([np.broadcast_to(x, (N, nw)) for x in transfers])                      # (S-1, N, NW)
    d_tr = t(np.ascontiguousarray(tr).view(np.float64).reshape(S - 1, N, 2 * nw).transpose(0, 2, 1))
    d_aend = torch.empty((2 * nw, N), dtype=torch.float64, device=dev)
    d_we, d_wm = torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    steps = [sp[1] for sp in spans]
    rows = sum(n // save_every + 1 for n in steps)
    d_traj = torch.full((rows, nw, ld, 2), -7.0, dtype=torch.float64, device=dev)
    ws_bytes = nat.pairs_chain_workspace_bytes(K, N)
    d_ws = torch.full((ws_bytes + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    nat.pairs_chain_device(stream=torch.cuda.current_stream().cuda_stream, n_pairs=K, n_points=N, n_steps=steps,
                           seg_len=[sp[0] for sp in spans], save_every=save_every, d_dbeta_soa=d_db.data_ptr(),
                           d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(),
                           d_transfer_soa=d_tr.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                           d_p_wave_end_soa=d_we.data_ptr(), d_p_wave_max_soa=d_wm.data_ptr(),
                           d_first_bad=d_bad.data_ptr(), d_traj_soa=d_traj.data_ptr(), d_workspace=d_ws.data_ptr())
    torch.cuda.synchronize()
    full = d_traj.cpu().numpy()                                                          # [rows][NW][ld][2]
    return dict(a_end=np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128), p_wave_end=d_we.cpu().numpy().T,
                p_wave_max=d_wm.cpu().numpy().T, first_bad_step=d_bad.cpu().numpy(),
                traj=np.ascontiguousarray(full[:, :, :N].transpose(2, 0, 1, 3)).view(np.complex128)[..., 0],
                pad=full[:, :, N:], guard=d_ws[ws_bytes:].cpu().numpy())


@pytest.mark.parametrize("N,K,steps,lengths", [(300, 3, (60, 100, 40), (300.0, 500.0, 200.0)), (131072, 1, (2, 3, 2), (1.0, 1.5, 1.0))],
                         ids=["300", "131072-padded"])
def test_device_entry_equals_the_host_entry_bit_for_bit(N, K, steps, lengths):
    """PSA_OPT_TRAJ_LD on the `_dev` form: ld = psa_traj_ld(N, 8), which is N for 300 points and N + 272 for 131 072.  The
    padding and the bytes behind the workspace are never written; a handful of the padded case's points also go against
    the restatement, which an epilogue that ignored the leading dimension would miss."""
    import torch
    se = 20 if N == 300 else 1
    ld = nat.traj_ld(N)
    assert ld == (N if N == 300 else N + 272)
    case = chain_np.lossy_case(N, K, steps=steps, lengths=lengths)
    a0, spans, transfers = case
    host = nat.pairs_chain_host(np.stack([sp[2] for sp in spans]), n_steps=steps, seg_len=lengths, save_every=se,
                                gamma=np.stack([sp[3] for sp in spans]), alpha=np.stack([sp[4] for sp in spans]), a0=a0,
                                transfers=np.stack([np.broadcast_to(x, a0.shape) for x in transfers]), want_traj=True)
    got = _device_chain(torch, a0, spans, transfers, save_every=se, flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_TRAJ_LD,
                        ld=ld)
    for key in KEYS + ("traj",):
        assert np.array_equal(got[key], host[key]), key
    assert np.all(got["pad"] == -7.0) and np.all(got["guard"] == 0x5A)
    idx = np.array([0, 1, 63, 64, 255, 256, N // 2, N - 2, N - 1])
    ref = chain_np.chain(*chain_np.subset(case, idx), se)
    assert wave_err(got["traj"][idx], ref["rows"]) < RTOL_F64 and power_err(got["p_wave_max"][idx], ref["p_wave_max"]) < RTOL_F64


def test_two_devices_equal_one():
    a0, spans, transfers = chain_np.lossy_case(41, 3, steps=(60, 100, 40))
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    one = rk4_chain_pairs(_fibre(spans), **kw)
    two = rk4_chain_pairs(_fibre(spans), devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (41, 4 + 6 + 3, 8)
    # the sweep's rows split the same way
    a0, db, gamma, alpha, _ = _one_span(3)
    kw = dict(z_max=260.0, n_steps=130, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    one, two = rk4_sweep_pairs(db, **kw), rk4_sweep_pairs(db, devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key


# ---- the phase scan -------------------------------------------------------------------------------------------------------
def test_phase_scan_driver_against_the_closed_form_and_a_direct_call():
    """The lossless WDM copier - PSA link of pairs_chain_np.wdm_case: K = 4 channels, 1e-12 W seeds, dark idlers, alpha = 0,
    F = 16 pump phases.  Every channel's gain is a_k + b_k cos(2 phi + const) with the dual-pump closed form (g_k^2 = 4 gamma^2
    P1 P2 - (kappa_k/2)^2, kappa_k = dbeta_k + gamma (P1 + P2)): DFT bin 0 and 2 |bin 2| meet a_k and b_k at BAR_BIN = 7.1e-8
    and every other bin stays below BAR_REST = 5.9e-10 of bin 0 -- ten times what the NumPy restatement leaves at the same
    step counts (tests/test_pairs_chain_host.py).  The scan equals the chain call it stands for to 1e-12."""
    c = chain_np.wdm_case()
    disp = dispersion.DispersionParams(**c["disp"])
    (Lc, Lp), (nc, npsa) = c["lengths"], c["steps"]
    kw = dict(psa_cfg=config.custom_simulation_config(z_max=Lp, dz=Lp / npsa, save_every=50),
              copier_cfg=config.custom_simulation_config(z_max=Lc, dz=Lc / nc, save_every=50), lambda_p1_m=c["lambda_p1_m"],
              lambda_p2_m=c["lambda_p2_m"], Omega=c["Omega"], p_pump=[c["p_pump"]] * 2, p_signal=[c["p_seed"]] * 4, p_idler=0.0,
              gamma=c["gamma"], alpha=0.0, dispersion=disp, phase=c["phases"], phase_wave="pumps", gain_mode="end")
    out = scan_mismtach.scan_wdm_copier_psa_phase(gain_unit="linear", **kw)
    assert out["gain"].shape == out["idler"].shape == (16, 4) and out["dbeta"].shape == (2, 4) and out["result"].n_steps == 500
    assert np.array_equal(out["dbeta"][0], out["dbeta"][1]) and np.all(out["first_bad_step"] == -1)
    a, b = chain_np.closed_form_gain(out["dbeta"][0], Lc, out["dbeta"][1], Lp, c["gamma"], c["p_pump"], c["p_pump"])
    for k in range(4):
        e0, e2, rest = chain_np.check_harmonics(out["gain"][:, k], a[k], b[k])
        print(f"channel {k}: gain {a[k]:.3f} +- {b[k]:.3f}; bin 0 {e0:.2e} bin 2 {e2:.2e} other bins {rest:.2e}")
        assert e0 < c["BAR_BIN"] and e2 < c["BAR_BIN"] and rest < c["BAR_REST"]
    # the idlers carry their signals' photons: P_i = P_s - P_s(0) in the lossless chain
    assert np.max(np.abs(out["idler"] - (out["gain"] - 1.0)) / out["gain"]) < 1e-9
    in_db = scan_mismtach.scan_wdm_copier_psa_phase(gain_unit="dB", **kw)
    assert np.max(np.abs(10.0 ** (in_db["gain"] / 10.0) / out["gain"] - 1.0)) < 1e-12
    for key, want in (("gain_max_db", in_db["gain"].max(axis=0)), ("gain_min_db", in_db["gain"].min(axis=0)),
                      ("extinction_db", in_db["gain"].max(axis=0) - in_db["gain"].min(axis=0))):
        assert out[key].shape == (4,) and np.array_equal(in_db[key], want) and np.array_equal(out[key], want), key
    # the chain call the scan stands for
    T = np.ones((16, 10), complex)
    T[:, :2] = np.exp(1j * c["phases"])[:, None]
    a_in = np.sqrt(np.array([c["p_pump"]] * 2 + [c["p_seed"], 0.0] * 4)).astype(complex)
    direct = rk4_chain_pairs([FibreSpan(Lc, n_steps=nc, dbeta=np.tile(out["dbeta"][0], (16, 1)), gamma=c["gamma"]),
                              FibreSpan(Lp, n_steps=npsa, dbeta=np.tile(out["dbeta"][1], (16, 1)), gamma=c["gamma"])],
                             a0=a_in, transfers=[T], save_every=50)
    assert wave_err(out["result"].a_end, direct.a_end) < 1e-12
    assert np.max(np.abs(out["gain"] / direct.channel_gain(np.full(4, c["p_seed"]), mode="end", unit="linear") - 1.0)) < 1e-12
