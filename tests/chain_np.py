"""The span loop of the three NumPy chain restatements (tests/single_pump_chain_np.py, pairs_chain_np.py, comb_chain_np.py):
one ``direct`` and one ``chain`` over a ``Model`` record that says what a family's span is.

* ``direct``: classic RK4 of the accumulated-phase model in the physical (A) frame.  Span s on its local coordinate zeta has
  the phases Theta_s + dbeta_s zeta, Theta_s = sum_{k<s} dbeta_k L_k, handed to the model's ``rhs``; the transfers act on A.
* ``chain``: the same chain span by span through the model's ``integrate`` (each span the plain model with its own mismatch
  and local z) in the B frame, B_s = A_s e^{+i Theta_s} on the gauged waves: a boundary is B' = T B with the gauged waves also
  times e^{+i dbeta_s L_s}; rows are brought back to A with e^{-i Theta_s}.  ``gauge=False`` leaves the boundary phase and the
  rotation out: the chain that forgot the gauge.

spans: (length, n_steps, mismatch, gamma, alpha) per span, gamma / alpha a scalar or (N,); the mismatch has the shape of the
gauged waves, for every point or with the points in front; transfers: S-1 entries (NW,) or (N, NW).
"""
import collections

import numpy as np

# integrate(b, mismatch, *, z_max, n, save_every, gamma, alpha) -> the family's dict with traj; rhs(theta, a, gamma, alpha) ->
# dA/dz with the phases theta in place of mismatch * z; gauged: the index of the waves that carry the accumulated phase (an int
# for one wave: its phase and mismatch are then (N,), not (N, 1))
Model = collections.namedtuple("Model", "integrate rhs gauged")


def _phase_shape(model, nw):
    return np.empty(nw)[model.gauged].shape


def _points(a0, spans, transfers=(), mismatch_ndim=2):
    """N of a case: the one size besides 1 among the per-point gamma / alpha, mismatches, transfers and a0."""
    sizes = {np.size(v) for sp in spans for v in sp[3:]} | {np.shape(x)[0] for x in list(transfers) if np.ndim(x) == 2}
    sizes |= {np.shape(sp[2])[0] for sp in spans if np.ndim(sp[2]) == mismatch_ndim}
    if np.ndim(a0) == 2:
        sizes.add(np.shape(a0)[0])
    sizes.discard(1)
    assert len(sizes) <= 1
    return sizes.pop() if sizes else 1


def _per_point(x, N):
    return np.array(np.broadcast_to(np.asarray(x, dtype=float), (N,)))


def _start(model, a0, spans, transfers):
    """-> N, the state (N, NW) and the zero phase of the gauged waves."""
    nw = np.shape(a0)[-1]
    shape = _phase_shape(model, nw)
    N = _points(a0, spans, transfers, 1 + len(shape))
    return N, np.array(np.broadcast_to(np.asarray(a0, dtype=np.complex128), (N, nw))), np.zeros((N,) + shape)


def direct(model, a0, spans, transfers, save_every):
    """-> rows (N, n_saved_total, NW) in the A frame: every span's row 0 (the post-transfer state) and a row after every
    save_every-th step."""
    N, y, theta0 = _start(model, a0, spans, transfers)
    rows = []
    for k, (L, n, db, g, al) in enumerate(spans):
        db = np.array(np.broadcast_to(np.asarray(db, dtype=float), theta0.shape))
        g, al = _per_point(g, N), _per_point(al, N)
        zg = np.linspace(0.0, L, n + 1)
        rows.append(y.copy())
        for i in range(n):
            z, h = zg[i], zg[i + 1] - zg[i]
            k1 = model.rhs(theta0 + db * z, y, g, al)
            k2 = model.rhs(theta0 + db * (z + 0.5 * h), y + 0.5 * h * k1, g, al)
            k3 = model.rhs(theta0 + db * (z + 0.5 * h), y + 0.5 * h * k2, g, al)
            k4 = model.rhs(theta0 + db * (z + h), y + h * k3, g, al)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            if (i + 1) % save_every == 0:
                rows.append(y.copy())
        if k + 1 < len(spans):
            y = y * np.asarray(transfers[k], dtype=np.complex128)
            theta0 = theta0 + db * L
    return np.stack(rows, axis=1)


def chain(model, a0, spans, transfers, save_every, gauge=True):
    """-> dict(rows (N, n_saved_total, NW) A frame, a_end (N, NW), p_wave_end, p_wave_max (N, NW) over every saved row,
    first_bad_step (N,) counted over the whole chain (first failure wins), z_out (n_saved_total,))."""
    N, b, theta = _start(model, a0, spans, transfers)
    bad = np.full(N, -1, dtype=np.int64)
    rows, z_out, z0, step0 = [], [], 0.0, 0
    for k, (L, n, db, g, al) in enumerate(spans):
        db = np.array(np.broadcast_to(np.asarray(db, dtype=float), theta.shape))
        r = model.integrate(b, db, z_max=L, n=n, save_every=save_every, gamma=g, alpha=al)
        A = r["traj"].copy()
        with np.errstate(all="ignore"):
            if gauge:
                A[:, :, model.gauged] *= np.exp(-1j * theta)[:, None]
            rows.append(A)
            z_out.append(z0 + np.linspace(0.0, L, n + 1)[::save_every])
            new = (bad < 0) & (r["first_bad_step"] >= 0)
            bad[new] = r["first_bad_step"][new] + step0
            z0, step0 = z0 + L, step0 + n
            if k + 1 < len(spans):
                b = r["a_end"] * np.asarray(transfers[k], dtype=np.complex128)
                if gauge:
                    b[:, model.gauged] *= np.exp(1j * db * L)
                    theta = theta + db * L
    rows = np.concatenate(rows, axis=1)
    with np.errstate(all="ignore"):
        p = np.abs(rows) ** 2
    return dict(rows=rows, a_end=rows[:, -1], p_wave_end=p[:, -1], p_wave_max=np.max(p, axis=1), first_bad_step=bad,
                z_out=np.concatenate(z_out))


def mid_stage(gain_db, phase):
    """sqrt(10^(gain_db/10)) e^{i phase}, written out here so the restatement does not lean on the package."""
    return np.sqrt(10.0 ** (np.asarray(gain_db, dtype=float) / 10.0)) * np.exp(1j * np.asarray(phase, dtype=float))


def subset(case, idx):
    """(a0, spans, transfers) of a lossy_case cut to the points ``idx``."""
    a0, spans, transfers = case
    return (a0[idx], [(L, n, db[idx], g[idx], al[idx]) for L, n, db, g, al in spans],
            [t[idx] if t.ndim == 2 else t for t in transfers])
