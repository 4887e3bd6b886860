"""What a fibre chain owes its caller in every wave-summary family, once: the single-pump, multi-channel and multi-line chains
(psa_rk4_single_pump_chain_f64, psa_rk4_pairs_chain_f64, psa_rk4_comb_chain_f64 and sweep.rk4_chain_*) share their span join,
epilogue and workspace in the library, so one test over the records of tests/wave_family.py guards them, against the NumPy
restatements at the project's bar RTOL_F64 (1e-9 of the point's largest wave):

* one fibre cut into 2, 3 and 7 spans with identity transfers is the unsplit sweep;
* a lossy three-span chain with per-point mismatch, gamma, alpha, a per-point and a broadcast transfer: 300 points cross a
  256-thread epilogue block and are no multiple of 64;
* spans of 1, 63, 64, 65 and 130 steps in one chain (the kernels re-seed their phases every 64 steps);
* the `_dev` entry on a caller's workspace of exactly the stated size and padded trajectory rows, bit-equal to the host form.
  psa_traj_ld pads only where the wave regions lie a multiple of 2 MiB apart, so 300 points have ld == N; the padded leading
  dimension is reached with 131 072 points on a chain of a few steps;
* devices=[0, 0] equals one device.

Every family keeps the inputs, widths and strides its own suite always had.  What only one family has stays in
tests/test_gpu_<family>_chain.py, and so do the two tests whose three forms differ in more than a flag: one span against the
sweep (three draws, and the multi-channel sweep returns no rows) and the failure in span two."""
import functools

import numpy as np
import pytest

import psa_amd._native as nat
from conftest import RTOL_F64
from psa_amd.sweep import FibreSpan
from wave_family import (COMB, KEYS, PAIRS, SINGLE_PUMP, case_id, comb_inputs, device_chain, fibre, lossy_case, pairs_inputs,
                         power_err, rows, single_pump_inputs, split, strided, wave_err)

pytestmark = pytest.mark.gpu


def cases(single_pump=(), pairs=(), comb=()):
    """(family, width) over the widths each family's suite runs a test at."""
    return [(f, w) for f, widths in ((SINGLE_PUMP, single_pump), (PAIRS, pairs), (COMB, comb)) for w in widths]


def over(**widths):
    """parametrize("family,width") over cases(**widths), ids as wave_family.case_id."""
    return pytest.mark.parametrize("family,width", [pytest.param(f, w, id=case_id(f, w)) for f, w in cases(**widths)])


# ---- identity split -------------------------------------------------------------------------------------------------------
UNSPLIT = {       # 33 points; the multi-channel suite runs K = 5 (three padding lanes)
    "single_pump": lambda _: single_pump_inputs(33, 2),
    "pairs": lambda K: pairs_inputs(33, K, 2, (0.9, 1.1), (0.5, 1.5)),
    "comb": lambda M: comb_inputs(33, M, 2 + M, (0.9, 1.1), (0.5, 1.5))}


@functools.lru_cache(maxsize=None)
def _unsplit(family, width):
    mm, a0, gamma, alpha = UNSPLIT[family.name](width)
    whole = family.rk4_sweep(mm, z_max=700.0, n_steps=1400, save_every=10, gamma=gamma, alpha=alpha, a0=a0, want_traj=True)
    return mm, a0, gamma, alpha, whole


@pytest.mark.parametrize("cuts", [2, 3, 7])
@over(single_pump=[None], pairs=[5], comb=[4, 12])
def test_identity_split_equals_the_unsplit_run(family, width, cuts):
    n_pts, n, L, se, nw = 33, 1400, 700.0, 10, family.n_waves(width)
    mm, a0, gamma, alpha, whole = _unsplit(family, width)
    steps = split(n, cuts, se)
    spans = [FibreSpan(L * s / n, n_steps=s, dbeta=mm, gamma=gamma, alpha=alpha) for s in steps]
    got = family.rk4_chain(spans, a0=a0, transfers=[np.ones(nw)] * (cuts - 1), save_every=se, want_traj=True)
    assert got.traj.shape == (n_pts, sum(s // se + 1 for s in steps), nw) and got.n_steps == n
    np.testing.assert_allclose(got.z_out, np.linspace(0, L, n + 1)[::se][rows(steps, se)], rtol=1e-12, atol=1e-9)

    def whole_err(a, b):            # the single-pump suite's measure: against the largest value of the whole array
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    both = dict(a_end=(got.a_end, whole.a_end), p_wave_end=(got.p_wave_end, whole.p_wave_end),
                p_wave_max=(got.p_wave_max, whole.p_wave_max), rows=(got.traj, whole.traj[:, rows(steps, se)]))
    errs = {k: (power_err if k.startswith("p_") else wave_err)(*v) for k, v in both.items()}
    errs.update({k + "/whole": whole_err(*v) for k, v in both.items()})
    print(f"{case_id(family, width)}, {cuts} spans against the unsplit sweep: "
          + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL_F64
    assert np.all(got.first_bad_step == -1)
    # without the trajectory the summaries are the same numbers
    lean = family.rk4_chain(spans, a0=a0, save_every=se)
    for key in KEYS:
        assert np.array_equal(getattr(lean, key), getattr(got, key)), key
    assert lean.traj is None


# ---- the lossy three-span chain -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lossy_reference(family, width):
    """300 points through the restatement once, every step saved; any save stride is read off the rows.  The single-pump
    suite runs the twin's own 600 + 1000 + 400 steps, the others 120 + 200 + 80."""
    case = lossy_case(family, width, 300, **({} if family is SINGLE_PUMP else dict(steps=(120, 200, 80))))
    ref = family.twin.chain(*case, 1)
    assert (ref["first_bad_step"] == -1).all()
    return case, ref["rows"], ref["z_out"]


@pytest.mark.parametrize("save_every", [1, 20])
@over(single_pump=[None], pairs=[3, 16], comb=[3, 7, 12])
def test_lossy_chain_with_transfers_against_the_restatement(family, width, save_every):
    (a0, spans, transfers), all_rows, z_all = _lossy_reference(family, width)
    want, z_want = strided(all_rows, z_all, [n for _, n, *_ in spans], save_every)
    got = family.rk4_chain(fibre(spans), a0=a0, transfers=transfers, save_every=save_every, want_traj=True)
    assert got.traj.shape == want.shape
    errs = (wave_err(got.traj, want), wave_err(got.a_end, want[:, -1]), power_err(got.p_wave_end, np.abs(want[:, -1]) ** 2),
            power_err(got.p_wave_max, np.max(np.abs(want) ** 2, axis=1)))
    print(f"lossy 3-span chain, {case_id(family, width)}, 300 points, save_every={save_every}: rows {errs[0]:.2e} "
          f"a_end {errs[1]:.2e} p_wave_end {errs[2]:.2e} p_wave_max {errs[3]:.2e}")
    assert max(errs) < RTOL_F64
    np.testing.assert_allclose(got.z_out, z_want, rtol=1e-14, atol=0.0)
    assert np.all(got.first_bad_step == -1) and np.array_equal(got.traj[:, -1], got.a_end)
    assert np.array_equal(got.row_offsets, np.concatenate([[0], np.cumsum([n // save_every + 1 for _, n, *_ in spans])]))


# ---- loop edges -------------------------------------------------------------------------------------------------------------
EDGES = {         # -> (metres per step, a span's mismatch drawn from rng)
    "single_pump": (0.5, lambda rng, N, _: rng.uniform(-4.5, 0.5, N) * 0.0115 * 0.5),
    "pairs": (2.0, lambda rng, N, K: rng.uniform(-3.5, 1.5, (N, K)) * PAIRS.twin.GAMMA * 2 * PAIRS.twin.P_PUMP),
    "comb": (2.0, lambda rng, N, M: COMB.twin.random_kappa(rng, N, M))}


@over(single_pump=[None], pairs=[3], comb=[4])
def test_loop_edges_in_one_chain(family, width):
    """Spans of 1, 63, 64, 65 and 130 steps, every step saved, per-point transfers between them."""
    N, steps, nw = 70, (1, 63, 64, 65, 130), family.n_waves(width)
    rng = np.random.default_rng(5)
    a0 = single_pump_inputs(N, 6)[1] if family is SINGLE_PUMP else family.twin.random_a0(rng, N, width)
    dz, mismatch = EDGES[family.name]
    spans = [(dz * n, n, mismatch(rng, N, width), 0.0115 * rng.uniform(0.9, 1.3, N), 1.15e-4 * rng.uniform(0.0, 2.0, N))
             for n in steps]
    transfers = [family.twin.mid_stage(rng.uniform(-2, 1, (N, nw)), rng.uniform(-np.pi, np.pi, (N, nw))) for _ in steps[1:]]
    ref = family.twin.chain(a0, spans, transfers, 1)
    got = family.rk4_chain(fibre(spans), a0=a0, transfers=transfers, save_every=1, want_traj=True)
    errs = (wave_err(got.traj, ref["rows"]), wave_err(got.a_end, ref["a_end"]), power_err(got.p_wave_max, ref["p_wave_max"]))
    print(f"loop edges, {case_id(family, width)}: rows {errs[0]:.2e} a_end {errs[1]:.2e} p_wave_max {errs[2]:.2e}")
    assert got.traj.shape == (N, sum(steps) + len(steps), nw) and max(errs) < RTOL_F64 and np.all(got.first_bad_step == -1)


# ---- the _dev entry -------------------------------------------------------------------------------------------------------
SHORT, PADDED = (300, (60, 100, 40), (300.0, 500.0, 200.0), 20), (131072, (2, 3, 2), (1.0, 1.5, 1.0), 1)


@pytest.mark.parametrize("family,width,N,steps,lengths,se", [
    pytest.param(f, w, *shape, id=f"{case_id(f, w)}-{'300' if shape[0] == 300 else '131072-padded'}") for f, w, shape in (
        (SINGLE_PUMP, None, SHORT), (SINGLE_PUMP, None, PADDED), (PAIRS, 3, SHORT), (PAIRS, 1, PADDED), (COMB, 4, SHORT),
        (COMB, 3, (131072, (20, 20), (10.0, 10.0), 10)))])
def test_device_entry_equals_the_host_entry_bit_for_bit(family, width, N, steps, lengths, se):
    """PSA_OPT_TRAJ_LD on the `_dev` form: ld = psa_traj_ld(N, 8), which is N for 300 points and N + 272 for 131 072.  The
    padding and the bytes behind the workspace are never written; a handful of the padded case's points also go against
    the restatement, which an epilogue that ignored the leading dimension would miss."""
    import torch
    ld = nat.traj_ld(N)
    assert ld == (N if N == 300 else N + 272)
    a0, spans, transfers = lossy_case(family, width, N, steps=steps, lengths=lengths)
    transfers = transfers[:len(steps) - 1]
    case = (a0, spans, transfers)
    host = family.chain_host(np.stack([sp[2] for sp in spans]), n_steps=steps, seg_len=lengths, save_every=se,
                             gamma=np.stack([sp[3] for sp in spans]), alpha=np.stack([sp[4] for sp in spans]), a0=a0,
                             transfers=np.stack([np.broadcast_to(x, a0.shape) for x in transfers]), want_traj=True)
    got = device_chain(torch, family, width, a0, spans, transfers, save_every=se,
                       flags=nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | nat.OPT_TRAJ_LD, ld=ld)
    for key in KEYS + ("traj",):
        assert np.array_equal(got[key], host[key]), key
    assert got["pad"].shape[2] == ld - N and np.all(got["pad"] == -7.0) and np.all(got["guard"] == 0x5A)
    idx = np.array([0, 1, 63, 64, 255, 256, N // 2, N - 2, N - 1])
    ref = family.twin.chain(*family.twin.subset(case, idx), se)
    assert wave_err(got["traj"][idx], ref["rows"]) < RTOL_F64 and power_err(got["p_wave_max"][idx], ref["p_wave_max"]) < RTOL_F64
    assert np.all(got["first_bad_step"] == -1)


# ---- devices ----------------------------------------------------------------------------------------------------------------
# the multi-channel suite keeps its own: it also splits the rows of a sweep over the devices
@over(single_pump=[None], comb=[5])
def test_two_devices_equal_one(family, width):
    a0, spans, transfers = lossy_case(family, width, 41, steps=(60, 100, 40))
    kw = dict(a0=a0, transfers=transfers, save_every=20, want_traj=True)
    one = family.rk4_chain(fibre(spans), **kw)
    two = family.rk4_chain(fibre(spans), devices=[0, 0], **kw)
    for key in KEYS + ("traj",):
        assert np.array_equal(getattr(one, key), getattr(two, key)), key
    assert one.traj.shape == (41, 4 + 6 + 3, family.n_waves(width))
