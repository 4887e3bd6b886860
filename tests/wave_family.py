"""What the GPU suites of the three wave-summary families (single-pump, multi-channel "pairs", multi-line "comb") share: the
error measures, the span bookkeeping, one record per family with the names that differ between them, and the `_dev` entries
driven from torch buffers.  A helper module imported by bare name, like the ``*_np`` restatements."""
import collections

import numpy as np

import comb_chain_np
import pairs_chain_np
import psa_amd._native as nat
import single_pump_chain_np
from psa_amd import sweep
from psa_amd.sweep import FibreSpan

KEYS = ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")


def wave_err(got, ref):
    """max |got - ref| over the largest wave of the point (amplitudes (N, ..., NW) complex)."""
    ref = np.asarray(ref)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (ref.ndim - 1))
    return float(np.max(np.abs(np.asarray(got) - ref) / scale))


def power_err(got, ref):
    """The same bar on a power summary (N, NW): the waves' moduli sqrt(P_j) against the point's largest."""
    return wave_err(np.sqrt(np.asarray(got)).astype(complex), np.sqrt(np.asarray(ref)).astype(complex))


# ---- spans and their saved rows -------------------------------------------------------------------------------------------
def fibre(spans):
    return [FibreSpan(L, n_steps=n, dbeta=db, gamma=g, alpha=al) for L, n, db, g, al in spans]


def split(n, cuts, se):
    """n steps cut into ``cuts`` spans of a multiple of ``se`` steps each, the last one taking the rest."""
    steps = np.full(cuts, (n // se // cuts) * se)
    steps[-1] = n - steps[:-1].sum()
    return [int(s) for s in steps]


def rows(steps, se):
    """The rows of the unsplit run (saved every ``se`` steps) that a chain of these spans saves: a boundary's row twice."""
    offs = np.concatenate([[0], np.cumsum(steps)[:-1]])
    return np.concatenate([o // se + np.arange(s // se + 1) for o, s in zip(offs, steps)])


def strided(rows, z_out, steps, se):
    """Rows of a chain saved every ``se`` steps, out of the rows saved at every step."""
    offs = np.concatenate([[0], np.cumsum(np.asarray(steps) + 1)[:-1]])
    idx = np.concatenate([o + np.arange(0, s - s % se + 1, se) for o, s in zip(offs, steps)])
    return rows[:, idx], z_out[idx]


# ---- the families ---------------------------------------------------------------------------------------------------------
# letter / count_arg: how the width (K pairs, M lines; None for the single pump) is written in a test id and in the head of a
# `_dev` call, in front of n_points; mismatch_arg: the `_dev` name of the mismatch, (S, N) or, in SoA, (S, width, N)
Family = collections.namedtuple("Family", "name letter n_waves twin sweep_host sweep_device chain_host chain_device "
                                          "chain_workspace_bytes rk4_sweep rk4_chain count_arg mismatch_arg")

SINGLE_PUMP = Family("single_pump", None, lambda _: 3, single_pump_chain_np, nat.single_pump_host, nat.single_pump_device,
                     nat.single_pump_chain_host, nat.single_pump_chain_device, nat.single_pump_chain_workspace_bytes,
                     sweep.rk4_sweep_single_pump, sweep.rk4_chain_single_pump, None, "d_dbeta")
PAIRS = Family("pairs", "K", lambda K: 2 + 2 * K, pairs_chain_np, nat.sweep_pairs_host, None, nat.pairs_chain_host,
               nat.pairs_chain_device, nat.pairs_chain_workspace_bytes, sweep.rk4_sweep_pairs, sweep.rk4_chain_pairs, "n_pairs",
               "d_dbeta_soa")
COMB = Family("comb", "M", lambda M: M, comb_chain_np, nat.comb_host, nat.comb_device, nat.comb_chain_host,
              nat.comb_chain_device, nat.comb_chain_workspace_bytes, sweep.rk4_sweep_comb, sweep.rk4_chain_comb, "n_lines",
              "d_kappa_soa")


def case_id(family, width):
    return family.name if width is None else f"{family.name}-{family.letter}{width}"


def lossy_case(family, width, N, **kw):
    """The twin's lossy_case: (a0, spans, transfers)."""
    return family.twin.lossy_case(N, *(() if width is None else (width,)), **kw)


# ---- the random points of each family's suite: -> mismatch (N,) or (N, width), a0, gamma, alpha -------------------------
def single_pump_inputs(N, seed):
    rng = np.random.default_rng(seed)
    dbeta = rng.uniform(-4.5, 0.5, N) * 0.0115 * 0.5
    p = np.column_stack([rng.uniform(0.3, 0.6, N), 10 ** rng.uniform(-8, -3, N), 10 ** rng.uniform(-8, -3, N)])
    a0 = np.sqrt(p) * np.exp(1j * rng.uniform(-3, 3, (N, 3)))
    return dbeta, a0, 0.0115 * rng.uniform(0.9, 1.1, N), 1.15e-4 * rng.uniform(0.5, 1.5, N)


def pairs_inputs(N, K, seed, gamma, alpha):
    tw = PAIRS.twin
    rng = np.random.default_rng(seed)
    a0 = tw.random_a0(rng, N, K)
    db = rng.uniform(-3.5, 1.5, (N, K)) * tw.GAMMA * 2 * tw.P_PUMP
    return db, a0, tw.GAMMA * rng.uniform(*gamma, N), 1.15e-4 * rng.uniform(*alpha, N)


def comb_inputs(N, M, seed, gamma, alpha):
    tw = COMB.twin
    rng = np.random.default_rng(seed)
    kp, a0 = tw.random_kappa(rng, N, M), tw.random_a0(rng, N, M)
    return kp, a0, tw.GAMMA * rng.uniform(*gamma, N), 1.15e-4 * rng.uniform(*alpha, N)


# ---- the `_dev` entries on torch buffers ----------------------------------------------------------------------------------
def _head(family, width, N):
    return dict({} if width is None else {family.count_arg: width}, n_points=N)


def _outputs(torch, dev, N, nw, n_rows, ld):
    """-> the output buffers of a `_dev` call as its keyword arguments (the trajectory pre-filled with -7.0, or none), and a
    function that reads them back as the host entry's dictionary with the trajectory's padding."""
    d_aend = torch.empty((2 * nw, N), dtype=torch.float64, device=dev)
    d_we, d_wm = torch.empty((nw, N), dtype=torch.float64, device=dev), torch.empty((nw, N), dtype=torch.float64, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    d_traj = None if ld is None else torch.full((n_rows, nw, ld, 2), -7.0, dtype=torch.float64, device=dev)

    def read():
        torch.cuda.synchronize()
        out = dict(a_end=np.ascontiguousarray(d_aend.cpu().numpy().T).view(np.complex128), p_wave_end=d_we.cpu().numpy().T,
                   p_wave_max=d_wm.cpu().numpy().T, first_bad_step=d_bad.cpu().numpy(), traj=None, pad=None)
        if d_traj is not None:
            full = d_traj.cpu().numpy()                                                  # [rows][NW][ld][2]
            out["traj"] = np.ascontiguousarray(full[:, :, :N].transpose(2, 0, 1, 3)).view(np.complex128)[..., 0]
            out["pad"] = full[:, :, N:]
        return out
    return dict(d_a_end_soa=d_aend.data_ptr(), d_p_wave_end_soa=d_we.data_ptr(), d_p_wave_max_soa=d_wm.data_ptr(),
                d_first_bad=d_bad.data_ptr(), d_traj_soa=(0 if d_traj is None else d_traj.data_ptr())), read


def device_sweep(torch, family, width, mismatch, gamma, alpha, a0, *, n_steps, z_max, save_every, flags, traj_ld=None):
    """The family's sweep `_dev` entry on torch buffers -> the host entry's dictionary (traj from a [rows][NW][ld][2] buffer)."""
    dev = torch.device("cuda:0")
    N, nw = a0.shape
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_mm, d_g, d_al = t(mismatch.T), t(np.atleast_1d(gamma)), t(np.atleast_1d(alpha))
    d_a0 = t(a0.view(np.float64).reshape(N, 2 * nw).T)
    outputs, read = _outputs(torch, dev, N, nw, n_steps // save_every + 1, traj_ld)
    family.sweep_device(stream=torch.cuda.current_stream().cuda_stream, **_head(family, width, N), n_steps=n_steps,
                        z_max=z_max, save_every=save_every, **{family.mismatch_arg: d_mm.data_ptr()},
                        d_gamma=d_g.data_ptr(), d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags, **outputs)
    return read()


def device_chain(torch, family, width, a0, spans, transfers, *, save_every, flags, ld):
    """The family's chain `_dev` entry on torch buffers with a workspace of exactly the stated size (and a guard behind it)
    -> the host entry's dictionary, the trajectory's padding and the guard."""
    dev = torch.device("cuda:0")
    (N, nw), S = a0.shape, len(spans)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_mm = t(np.moveaxis(np.stack([sp[2] for sp in spans]), 1, -1))                      # (S, N) or (S, width, N)
    d_g, d_al = (t(np.stack([sp[k] for sp in spans])) for k in (3, 4))
    d_a0 = t(a0.view(np.float64).reshape(N, 2 * nw).T)
    tr = np.stack([np.broadcast_to(x, (N, nw)) for x in transfers])                      # (S-1, N, NW)
    d_tr = t(np.ascontiguousarray(tr).view(np.float64).reshape(S - 1, N, 2 * nw).transpose(0, 2, 1))
    steps = [sp[1] for sp in spans]
    outputs, read = _outputs(torch, dev, N, nw, sum(n // save_every + 1 for n in steps), ld)
    head = _head(family, width, N)
    ws_bytes = family.chain_workspace_bytes(*head.values())
    d_ws = torch.full((ws_bytes + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    family.chain_device(stream=torch.cuda.current_stream().cuda_stream, **head, n_steps=steps, seg_len=[sp[0] for sp in spans],
                        save_every=save_every, **{family.mismatch_arg: d_mm.data_ptr()}, d_gamma=d_g.data_ptr(),
                        d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), d_transfer_soa=d_tr.data_ptr(), flags=flags,
                        d_workspace=d_ws.data_ptr(), **outputs)
    return dict(read(), guard=d_ws[ws_bytes:].cpu().numpy())
