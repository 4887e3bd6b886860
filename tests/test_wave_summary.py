"""The per-wave power summary without a GPU: argument rules of psa_rk4_sweep_waves_* (PSA_E_FLAGS before any device work),
the public call surface of the touched drivers, and the sharded drivers carrying the per-wave columns through their one
all_gather (CPU, ``gloo``, world 2 and 3) -- equal to the unsharded call, in point order.

As in tests/test_driver_sharding_gloo.py the product executor is the HIP kernel, so inside the CPU-only workers the native
sweep is replaced by a test double built on the oracle: the per-wave rows are formed from the saved rows oracle.integrate
returns for each point."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import psa_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_FLAGS, E_NULLPTR = -11, -6


def _ptrs():
    buf = np.zeros(256)
    return buf, buf.ctypes.data_as(C.c_void_p)


def _waves_dev(flags=0, *, n_waves=4, traj=False, dtype="f64", dbeta2=False, waves_ptr=True):
    buf, p = _ptrs()
    fn = nat.lib().psa_rk4_sweep_waves_f64_dev if dtype == "f64" else nat.lib().psa_rk4_sweep_waves_f32_dev
    w = p if waves_ptr else None
    return fn(None, n_waves, 8, 10, 1.0, 1, p, p if dbeta2 else None, p, p, p, flags, p, p, p, p, p if traj else None, w, w)


def _waves_host(flags=0, *, traj=False, dtype="f64"):
    buf, p = _ptrs()
    fn = nat.lib().psa_rk4_sweep_waves_f64 if dtype == "f64" else nat.lib().psa_rk4_sweep_waves_f32
    return fn(0, 4, 8, 10, 1.0, 1, p, None, p, p, p, flags, p, p, p, p, p if traj else None, None, p, p)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", ["traj", "lds", "block64", "split+one", "quad+split", "quad6", "f32both"])
def test_waves_entry_points_reject_flags_before_device_work(dtype, case):
    """Without a GPU a call that passed validation would fail with PSA_E_DEVICE / a hipError_t: PSA_E_FLAGS proves the
    check comes first, on both faces."""
    kw = dict(flags=0, dtype=dtype)
    dev_kw = {}
    if case == "traj":
        kw["traj"] = True
    elif case == "lds":
        kw["flags"] = nat.OPT_LDS_STAGING
    elif case == "block64":
        kw["flags"] = nat.OPT_BLOCK64
    elif case == "split+one":
        kw["flags"] = nat.OPT_SPLIT_POINT | nat.OPT_ONE_LANE
    elif case == "quad+split":
        kw["flags"] = nat.OPT_QUAD_POINT | nat.OPT_SPLIT_POINT
    elif case == "quad6":
        kw["flags"] = nat.OPT_QUAD_POINT
        dev_kw = dict(n_waves=6, dbeta2=True)
    else:
        kw["flags"] = nat.OPT_F32_SCALAR | nat.OPT_F32_PACKED
    assert _waves_dev(**kw, **dev_kw) == E_FLAGS
    assert len(nat.lib().psa_last_error()) > 0
    if case != "quad6":
        assert _waves_host(**kw) == E_FLAGS


def test_waves_entry_points_need_both_wave_buffers():
    assert _waves_dev(waves_ptr=False) == E_NULLPTR
    buf, p = _ptrs()
    assert nat.lib().psa_rk4_sweep_waves_f64(0, 4, 8, 10, 1.0, 1, p, None, p, p, p, 0, p, p, p, p, None, None, None,
                                             None) == E_NULLPTR
    # an empty sweep stays a valid no-op
    assert nat.lib().psa_rk4_sweep_waves_f64(0, 4, 0, 10, 1.0, 1, None, None, None, None, None, 0, None, None, None, None,
                                             None, None, None, None) == 0


def test_python_faces_reject_a_trajectory_with_the_wave_summary():
    with pytest.raises(nat.PsaNativeError) as e:
        nat.sweep_host([0.0, 0.1], n_steps=10, z_max=1.0, save_every=1, gamma=1.0, alpha=0.0,
                       a0=np.ones(4, dtype=complex), want_traj=True, wave_summary=True)
    assert e.value.code == E_FLAGS


def test_summary_of_another_wave_needs_the_wave_columns():
    from psa_amd.sweep import SweepResult
    r = SweepResult(np.ones((2, 4), complex), np.ones(2), np.ones(2), -np.ones(2, np.int64), 10, 1, 0.0)
    assert r.p_wave_end is None and r.p_wave_max is None         # trailing optional fields, default None
    with pytest.raises(ValueError):
        r.summary(1.0, wave=3)


def test_call_surface_prefix_rule_still_holds_for_the_touched_drivers():
    """tests/golden/api_signatures.json: the reference's parameters are a prefix of the touched drivers' (new parameters
    only trail), and the dead upstream name stays absent."""
    import importlib
    import inspect
    import json
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "api_signatures.json")))
    mod = importlib.import_module("psa_amd.scan_mismtach")
    assert not hasattr(mod, "scan_mismatch_seeded_signal")
    checked = 0
    for modname in ("scan_mismtach", "simulation", "integrators"):
        m = importlib.import_module("psa_amd." + modname)
        for name, want in spec.get(modname, {}).items():
            if want["kind"] != "function" or not hasattr(m, name):
                continue
            got = [[n, q.kind.name, repr(q.default) if q.default is not inspect._empty else "<required>"]
                   for n, q in inspect.signature(getattr(m, name)).parameters.items()]
            assert got[:len(want["params"])] == want["params"], name
            checked += 1
    assert checked >= 3
    sig = inspect.signature(mod.scan_dbeta_seeded_signal).parameters
    assert list(sig)[-1] == "with_idler" and sig["with_idler"].default is False
    sig = inspect.signature(mod.seeded_mismatch_scan).parameters
    assert list(sig) == ["gain_mode", "device", "devices", "verbose"] and sig["gain_mode"].default == "end"


# ---- sharded drivers ------------------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _install_cpu_executor():
    """Test double for the host entry points, on the oracle (tests only); the per-wave rows come from each point's saved
    rows (oracle.integrate)."""
    import oracle as O

    def sweep_host(dbeta, *, n_steps, z_max, save_every, gamma, alpha, a0, dbeta2=None, check_nan=True, exact_step=False,
                   want_traj=False, dtype=np.float64, device=0, extra_flags=0, wave_summary=False):
        db = np.asarray(dbeta, dtype=np.float64)
        r = O.sweep(db, z_max=z_max, n=n_steps, save_every=save_every, check_nan=check_nan, gamma=gamma, alpha=alpha,
                    a0=a0, dbeta2=dbeta2, threads=1)
        r.update(traj=None, elapsed_ms=1.0, p_wave_end=None, p_wave_max=None)
        if wave_summary:
            a0v, g, a = np.asarray(a0), np.broadcast_to(gamma, db.shape), np.broadcast_to(alpha, db.shape)
            rows = [O.integrate(a0v if a0v.ndim == 1 else a0v[k], z_max=z_max, n=n_steps, save_every=save_every,
                                check_nan=check_nan, gamma=float(g[k]), alpha=float(a[k]), dbeta=float(db[k]))[1]
                    for k in range(db.size)]
            P = [np.abs(A) ** 2 for A in rows]
            r.update(p_wave_end=np.array([p[-1] for p in P]), p_wave_max=np.array([p.max(axis=0) for p in P]))
        return r

    def gain_summary_host(p_metric, first_bad_step, p0_sig, *, gain_db=True, device=0):
        g = O.gain_from_summary(p_metric, first_bad_step, p0_sig, "db" if gain_db else "linear")
        fin = np.isfinite(g)
        bi = int(np.nanargmax(g)) if fin.any() else -1
        return g, bi, (float(g[bi]) if bi >= 0 else float("nan")), int(fin.sum())

    nat.sweep_host, nat.gain_summary_host = sweep_host, gain_summary_host


def _scan(mode):
    from psa_amd import config, scan_mismtach
    cfg = config.custom_simulation_config(z_max=200.0, dz=1.0, save_every=5)
    out = scan_mismtach.scan_dbeta_seeded_signal(cfg=cfg, delta_beta=np.linspace(-0.05, 0.05, 25), gamma=0.0115,
                                                 alpha=1.15e-4, p_in=[0.5, 0.5, 1e-5, 1e-6], gain_mode=mode,
                                                 gain_unit="linear", with_idler=True)
    r = out["result"]
    return dict(gain=out["gain"], gain_idler=out["gain_idler"], best_gain_idler=out["best_gain_idler"],
                best_index=out["best_index"], p_wave_metric=out["p_wave_metric"], p_wave_end=r.p_wave_end,
                p_wave_max=r.p_wave_max, p_end=r.p_end, p_max=r.p_max)


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    _install_cpu_executor()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {f"{m}_{k}": v for m in ("end", "max") for k, v in _scan(m).items()}
    finally:
        dist.destroy_process_group()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_seeded_scan_carries_the_wave_columns_in_point_order(world, tmp_path):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    saved = nat.sweep_host, nat.gain_summary_host
    try:
        _install_cpu_executor()
        whole = {f"{m}_{k}": v for m in ("end", "max") for k, v in _scan(m).items()}
    finally:
        nat.sweep_host, nat.gain_summary_host = saved
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        assert set(got.files) == set(whole)
        for k, v in whole.items():
            np.testing.assert_array_equal(got[k], v, err_msg=f"rank {r}: {k}")
    for m in ("end", "max"):
        pw = whole[f"{m}_p_wave_metric"]
        assert pw.shape == (25, 4)
        # wave 2's column is the signal's own summary (bit for bit on the GPU; the double forms |A|^2 two ways), wave 3's
        # over p_in[2] is the idler gain
        np.testing.assert_allclose(pw[:, 2], whole[f"{m}_p_{m}"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(whole[f"{m}_gain_idler"], pw[:, 3] / 1e-5, rtol=1e-15, atol=0)
        assert whole[f"{m}_best_gain_idler"] == whole[f"{m}_gain_idler"][int(whole[f"{m}_best_index"])]
    # the pumps deplete: their maximum is the launch power, their end value below it
    assert np.all(whole["max_p_wave_metric"][:, :2] >= whole["end_p_wave_metric"][:, :2])
