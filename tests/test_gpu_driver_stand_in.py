"""The stand-in of tests/golden/driver_parent_cases.py has the real wrappers' shapes: for each of the eight host functions of
_native the drivers call, one real launch and the stand-in's answer to the same arguments agree in keys, dtypes, shapes and in
what is None.  No values are compared: tests/test_driver_parent.py holds the drivers over the stand-in, this holds the stand-in.

3 points in float64, 5 in float32 for the two packed kernels (an odd count: two points per lane); 20 steps saved every tenth,
with the rows and without; K = 1 pair, M = 3 lines, and two spans (20 and 30 steps) for the chains."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import driver_parent_cases as DC  # noqa: E402
import psa_amd._native as nat  # noqa: E402

pytestmark = pytest.mark.gpu


def _a0(N, nw, cplx=np.complex128):
    rng = np.random.default_rng(7)
    p = np.full((N, nw), 1e-4)
    p[:, :1] = 0.4
    return (np.sqrt(p) * np.exp(1j * rng.uniform(-1.0, 1.0, (N, nw)))).astype(cplx)


def _sweep(N, cols, **extra):
    """Arguments of a sweep wrapper: N points, a mismatch of ``cols`` columns (None: 1-D)."""
    mis = np.linspace(-0.3, 0.2, N * (cols or 1)).reshape((N, cols) if cols else (N,))
    return mis, dict(n_steps=20, z_max=2.0, save_every=10, gamma=1.1, alpha=1.15e-2, **extra)


def _chain(N, cols, nw, **extra):
    """Arguments of a chain wrapper: two spans of 20 and 30 steps, a per-point transfer between them."""
    mis = np.linspace(-0.3, 0.2, 2 * N * (cols or 1)).reshape((2, N, cols) if cols else (2, N))
    return mis, dict(n_steps=[20, 30], seg_len=[2.0, 3.0], save_every=10, gamma=np.array([1.1, 1.3]), alpha=np.array([1.15e-2, 0.0]),
                     a0=_a0(N, nw), transfers=np.full((1, N, nw), 0.9 + 0.1j), **extra)


def _cases():
    f32 = dict(dtype=np.float32)
    yield "sweep_pairs_host", _sweep(3, 1, a0=_a0(3, 4))
    for rows in (False, True):
        yield "single_pump_host", _sweep(3, None, a0=_a0(3, 3), want_traj=rows)
        yield "single_pump_host", _sweep(5, None, a0=_a0(5, 3, np.complex64), want_traj=rows, **f32)
        yield "comb_host", _sweep(3, 3, a0=_a0(3, 3), want_traj=rows)
        yield "comb_host", _sweep(5, 3, a0=_a0(5, 3, np.complex64), want_traj=rows, **f32)
        yield "chain_host", _chain(3, None, 4, want_traj=rows, wave_summary=not rows)    # the per-wave summary takes no rows
        yield "chain_host", _chain(3, None, 4, want_traj=rows, **f32)
        yield "single_pump_chain_host", _chain(3, None, 3, want_traj=rows)
        yield "pairs_chain_host", _chain(3, 1, 4, want_traj=rows)
        yield "comb_chain_host", _chain(3, 3, 3, want_traj=rows)


def _form(x):
    if isinstance(x, dict):
        return {k: _form(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return tuple(_form(v) for v in x)
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape)
    return type(x).__name__


CASES = list(_cases())


@pytest.mark.parametrize("name,call", CASES, ids=[f"{name}-{i}" for i, (name, _) in enumerate(CASES)])
def test_a_real_launch_has_the_stand_ins_form(name, call):
    mismatch, kw = call
    got = getattr(nat, name)(mismatch, **kw)
    want = getattr(DC.StandIn(), name)(mismatch, **kw)
    assert _form(got) == _form(want)
    assert (got["first_bad_step"] == -1).all()


@pytest.mark.parametrize("real,N", [(np.float64, 3), (np.float32, 5)])
@pytest.mark.parametrize("bad", [False, True])
def test_the_gain_summary_has_the_stand_ins_form(real, N, bad):
    p = np.linspace(0.5, 2.0, N).astype(real)
    first_bad = np.array([-1, 4] + [-1] * (N - 2), dtype=np.int64) if bad else None
    got = nat.gain_summary_host(p, first_bad, 1e-2, gain_db=True)
    want = DC.StandIn().gain_summary_host(p, first_bad, 1e-2, gain_db=True)
    assert _form(got) == _form(want)
