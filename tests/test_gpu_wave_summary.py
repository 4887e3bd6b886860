"""The per-wave power summary on hardware (psa_rk4_sweep_waves_*, SweepResult.p_wave_end / p_wave_max,
scan_dbeta_seeded_signal(with_idler=True), seeded_mismatch_scan):

* bit-equality with psa_rk4_sweep_* in every layout -- one lane, two lanes, four lanes (forced and automatic), float32 scalar
  and packed -- for 4 and 6 waves, lossy and lossless, check modes none / block / exact: a_end, first_bad_step and the wave-2
  columns equal p_end / p_max bit for bit;
* every wave against an independent source: the maximum and last row of the trajectory of the same launch;
* against the reference (tests/golden/G16.npz, tests/golden/gen_golden_waves.py): its repaired seeded mismatch scan, a lossy
  scan with a seeded idler, and points past the stability edge (NaN masks);
* the sharded driver: three ranks share the GPU over gloo and return the unsharded call's numbers."""
import os
import socket
import sys

import numpy as np
import pytest

from conftest import RTOL_F64, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

import psa_amd._native as nat  # noqa: E402

CHECKS = {"none": dict(check_nan=False), "block": dict(check_nan=True, exact_step=False),
          "exact": dict(check_nan=True, exact_step=True)}


def _case(nw, lossy, dtype):
    """37 points (odd: the packed kernel's tail), two of them past the stability edge; 1000 steps saved every 7 (a tail)."""
    n = 37
    db = np.linspace(-0.05, 0.05, n)
    gamma = np.full(n, 0.0115)
    gamma[[5, 30]] = 300.0
    p = [0.5, 0.5, 1e-5, 1e-5] if nw == 4 else [0.3, 0.25, 1e-6, 1e-6, 2e-6, 5e-7]
    a0 = np.sqrt(np.array(p)).astype(complex) * np.exp(1j * np.linspace(0.1, 0.7, nw))
    kw = dict(n_steps=1000, z_max=100.0, save_every=7, gamma=gamma, alpha=(1.15e-4 if lossy else 0.0), a0=a0, dtype=dtype)
    if nw == 6:
        kw["dbeta2"] = np.linspace(0.03, -0.02, n)
    return db, kw


F64_LAYOUTS = {"auto": 0, "one": nat.OPT_ONE_LANE, "split": nat.OPT_SPLIT_POINT, "quad": nat.OPT_QUAD_POINT}
F32_LAYOUTS = {"auto": 0, "scalar": nat.OPT_F32_SCALAR, "packed": nat.OPT_F32_PACKED}
CASES = ([("f64", lay, nw) for lay in F64_LAYOUTS for nw in (4, 6) if not (lay == "quad" and nw == 6)]
         + [("f32", lay, nw) for lay in F32_LAYOUTS for nw in (4, 6)])


@pytest.mark.parametrize("check", list(CHECKS))
@pytest.mark.parametrize("lossy", [True, False])
@pytest.mark.parametrize("prec,layout,nw", CASES)
def test_wave_summary_is_bit_equal_to_the_existing_entry_point(prec, layout, nw, lossy, check):
    dtype = np.float64 if prec == "f64" else np.float32
    flags = (F64_LAYOUTS if prec == "f64" else F32_LAYOUTS)[layout]
    db, kw = _case(nw, lossy, dtype)
    kw.update(CHECKS[check])
    ref = nat.sweep_host(db, extra_flags=flags, **kw)
    got = nat.sweep_host(db, extra_flags=flags, wave_summary=True, **kw)
    assert ref["p_wave_end"] is None and got["p_wave_end"].shape == (db.size, nw) and got["p_wave_max"].dtype == dtype
    np.testing.assert_array_equal(got["a_end"], ref["a_end"])
    np.testing.assert_array_equal(got["first_bad_step"], ref["first_bad_step"])
    np.testing.assert_array_equal(got["p_end"], ref["p_end"])
    np.testing.assert_array_equal(got["p_max"], ref["p_max"])
    # bit for bit, NaN in the same places (assert_array_equal treats NaN == NaN)
    np.testing.assert_array_equal(got["p_wave_end"][:, 2], ref["p_end"])
    np.testing.assert_array_equal(got["p_wave_max"][:, 2], ref["p_max"])
    # the failing points are non-finite in every wave; the others finite
    bad = ~np.isfinite(ref["a_end"]).all(axis=1)
    assert bad[[5, 30]].all() and not bad[[0, 18, 36]].any()
    assert (~np.isfinite(got["p_wave_max"][bad])).all() and np.isfinite(got["p_wave_max"][~bad]).all()


@pytest.mark.parametrize("layout", list(F64_LAYOUTS))
@pytest.mark.parametrize("nw", [4, 6])
@pytest.mark.parametrize("lossy", [True, False])
def test_every_wave_against_the_trajectory_of_the_same_launch(layout, nw, lossy):
    if layout == "quad" and nw == 6:
        pytest.skip("four lanes per point exist for the 4-wave model only")
    db, kw = _case(nw, lossy, np.float64)
    kw["gamma"] = 0.0115                                   # all points finite
    flags = F64_LAYOUTS[layout]
    got = nat.sweep_host(db, extra_flags=flags, wave_summary=True, **kw)
    tr = nat.sweep_host(db, extra_flags=flags, want_traj=True, **kw)["traj"]     # (N, n_saved, nw)
    P = tr.real ** 2 + tr.imag ** 2
    assert rel_err(got["p_wave_max"], P.max(axis=1)) <= 1e-15
    assert rel_err(got["p_wave_end"], P[:, -1, :]) <= 1e-15
    # the pumps deplete and the sidebands grow somewhere in this sweep: each wave's maximum is its own
    assert (got["p_wave_max"][:, 0] > got["p_wave_end"][:, 0]).any() and (got["p_wave_max"][:, 2] > P[:, 0, 2]).any()


def _g16():
    return np.load(os.path.join(GOLDEN, "G16.npz"))


@pytest.mark.parametrize("layout", ["auto", "one", "split", "quad"])
def test_lossy_seeded_idler_against_the_reference(layout):
    g = _g16()
    p_in = g["p_in"]
    kw = dict(n_steps=int(g["lossy_n_steps"]), z_max=float(g["lossy_z_max"]), save_every=int(g["lossy_save_every"]),
              gamma=float(g["lossy_gamma"]), alpha=float(g["lossy_alpha"]), a0=np.sqrt(p_in).astype(complex))
    got = nat.sweep_host(g["lossy_dbeta"], extra_flags=F64_LAYOUTS[layout], wave_summary=True, **kw)
    assert rel_err(got["p_wave_end"], g["lossy_p_wave_end"]) < RTOL_F64
    assert rel_err(got["p_wave_max"], g["lossy_p_wave_max"]) < RTOL_F64
    # the running maximum is exercised for every wave: pumps at z = 0, signal and idler later
    ref_max = g["lossy_p_wave_max"]
    assert rel_err(ref_max[:, :2], np.broadcast_to(p_in[:2], (ref_max.shape[0], 2))) < 1e-15   # |A(0)|^2 up to rounding
    assert np.all(ref_max[:, :2] > g["lossy_p_wave_end"][:, :2]) and (ref_max[:, 2:] > 1.01 * p_in[2:]).any()
    for flags in (nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED):
        g32 = nat.sweep_host(g["lossy_dbeta"], extra_flags=flags, wave_summary=True, dtype=np.float32, **kw)
        for key in ("p_wave_end", "p_wave_max"):
            ref = g["lossy_" + key]
            err = np.abs(g32[key].astype(np.float64) - ref) / ref.max(axis=1, keepdims=True)
            assert err.max() < 1e-3, (flags, key, err.max())


@pytest.mark.parametrize("check", list(CHECKS))
def test_failing_points_have_the_reference_nan_masks(check):
    g = _g16()
    kw = dict(n_steps=int(round(float(g["fail_z_max"]) / float(g["fail_dz"]))), z_max=float(g["fail_z_max"]),
              save_every=int(g["fail_save_every"]), gamma=g["fail_gammas"], alpha=0.0,
              a0=np.sqrt(g["p_in"]).astype(complex), **CHECKS[check])
    dbeta = np.full(g["fail_gammas"].size, float(g["fail_dbeta"]))
    for flags in (0, nat.OPT_ONE_LANE, nat.OPT_SPLIT_POINT, nat.OPT_QUAD_POINT):
        got = nat.sweep_host(dbeta, extra_flags=flags, wave_summary=True, **kw)
        for key in ("p_wave_end", "p_wave_max"):
            ref = g["fail_" + key]
            np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(ref), err_msg=f"{flags} {key}")
            fin = np.isfinite(ref)
            assert rel_err(got[key][fin], ref[fin]) < RTOL_F64
    clear = np.isin(g["fail_gammas"], [50.0, 200.0, 1e3, 10.0])      # far from the edge: float32 fails (or not) alike
    for flags in (nat.OPT_F32_SCALAR, nat.OPT_F32_PACKED):
        k32 = dict(kw, gamma=g["fail_gammas"][clear])
        got = nat.sweep_host(dbeta[clear], extra_flags=flags, wave_summary=True, dtype=np.float32, **k32)
        np.testing.assert_array_equal(np.isnan(got["p_wave_max"]), np.isnan(g["fail_p_wave_max"][clear]))


@pytest.mark.parametrize("mode", ["end", "max"])
def test_seeded_mismatch_scan_against_the_reference(mode, capsys):
    from psa_amd import scan_mismtach
    g = _g16()
    out = scan_mismtach.seeded_mismatch_scan(mode, verbose=True)
    printed = capsys.readouterr().out
    np.testing.assert_array_equal(out["delta"], g["seed_delta"])
    assert out["best_index"] == int(g[f"seed_{mode}_best_idx"])
    assert rel_err(out["Gs"], g[f"seed_{mode}_Gs"]) < RTOL_F64
    assert rel_err(out["Gi"], g[f"seed_{mode}_Gi"]) < RTOL_F64
    assert rel_err(out["p_wave_metric"], g[f"seed_p_wave_{mode}"]) < RTOL_F64
    bi = int(g[f"seed_{mode}_best_idx"])
    assert abs(out["best_Gs"] / g[f"seed_{mode}_Gs"][bi] - 1) < RTOL_F64
    assert abs(out["best_Gi"] / g[f"seed_{mode}_Gi"][bi] - 1) < RTOL_F64
    assert "=== Mismatch scan results ===" in printed
    assert f"best_delta = {float(g['seed_delta'][bi]):.6g} 1/km" in printed
    assert f"= {float(g[f'seed_{mode}_Gs'][bi]):.6g}" in printed and f"= {float(g[f'seed_{mode}_Gi'][bi]):.6g}" in printed


def test_seeded_scan_with_idler_and_summary_of_any_wave():
    from psa_amd import config, scan_mismtach
    cfg = config.custom_simulation_config(z_max=200.0, dz=0.1)
    p_in = [0.5, 0.5, 1e-5, 1e-6]
    for mode in ("end", "max"):
        out = scan_mismtach.scan_dbeta_seeded_signal(cfg=cfg, delta_beta=np.linspace(-0.05, 0.05, 101), gamma=0.0115,
                                                     alpha=1.15e-4, p_in=p_in, gain_mode=mode, gain_unit="linear",
                                                     with_idler=True)
        r = out["result"]
        col = r.p_wave_max if mode == "max" else r.p_wave_end
        np.testing.assert_array_equal(out["p_wave_metric"], col)
        np.testing.assert_array_equal(col[:, 2], r.p_max if mode == "max" else r.p_end)
        assert rel_err(out["gain_idler"], col[:, 3] / p_in[2]) <= 4e-16
        assert out["best_gain_idler"] == out["gain_idler"][out["best_index"]]
        for w in range(4):
            g, _, _, _ = r.summary(p_in[w], mode=mode, unit="linear", wave=w)
            assert rel_err(g, col[:, w] / p_in[w]) <= 4e-16


def _sharded_calls():
    from psa_amd import config, scan_mismtach
    cfg = config.custom_simulation_config(z_max=200.0, dz=0.1)
    out = {}
    for mode in ("end", "max"):
        r = scan_mismtach.scan_dbeta_seeded_signal(cfg=cfg, delta_beta=np.linspace(-0.05, 0.05, 101), gamma=0.0115,
                                                   alpha=1.15e-4, p_in=[0.5, 0.5, 1e-5, 1e-6], gain_mode=mode,
                                                   with_idler=True)
        out.update({f"{mode}_gain": r["gain"], f"{mode}_gain_idler": r["gain_idler"],
                    f"{mode}_best_gain_idler": r["best_gain_idler"], f"{mode}_p_wave_metric": r["p_wave_metric"],
                    f"{mode}_p_wave_end": r["result"].p_wave_end, f"{mode}_p_wave_max": r["result"].p_wave_max})
    s = scan_mismtach.seeded_mismatch_scan("max")
    out.update(seed_Gs=s["Gs"], seed_Gi=s["Gi"], seed_p=s["p_wave_metric"], seed_best=s["best_index"])
    return out


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **_sharded_calls())
    finally:
        dist.destroy_process_group()


def test_three_ranks_share_the_gpu_and_return_the_unsharded_wave_columns(tmp_path):
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_worker, args=(3, port, str(tmp_path)), nprocs=3, join=True)
    r = [np.load(tmp_path / f"r{k}.npz") for k in range(3)]
    whole = _sharded_calls()                     # this process: no process group, one launch per call
    for k in range(3):
        assert set(r[k].files) == set(whole)
        for key in whole:
            # small sweeps: the same lane layout (four lanes per point) in every block and in the whole launch
            assert np.array_equal(r[k][key], whole[key], equal_nan=True), (k, key)
