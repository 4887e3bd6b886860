"""The cases of tests/test_gpu_wave_family_parent.py, shared with gen_golden_wave_family_parent.py (which records
wave_family_parent.npz): the three wave-summary families -- the multi-channel ("pairs"), single-pump and multi-line ("comb")
sweeps -- as the library returned them before they shared one host path.

The smallest launches that reach every line the families share from the C entry points up: K = 1, 3, 16 pairs (2, 4 and 16
lanes per point) and M = 3, 5, 12 lines; N = 5 and 67 points in float64, 5 and 131 in float32 (two points per lane: an odd
count and a partial second wave); 40 steps saved every step or every tenth and 45 steps saved every tenth (a tail behind the
last saved row); gamma, alpha and a0 broadcast and per point, a broadcast alpha of exactly 0 and a per-point alpha holding
one; with and without the saved rows (at 5 points only, and for the pairs through pairs_chain_host with one span, as
rk4_sweep_pairs(want_traj=True) calls it); a point that goes non-finite, with the exact and the per-block step index; every
family's `_dev` entry point on torch buffers with and without PSA_OPT_TRAJ_LD and rows; and one two-span chain of the pairs
and of the comb.  Every launch draws its inputs from the same 131 points; a case with rows has the inputs of the one without,
so their summaries are stored once (chain_parent_cases.pack)."""
import numpy as np

from chain_parent_cases import pack, unpack  # noqa: F401  (the record's format is chain_parent.npz's)

N_ALL = 131
DZ = 0.1
BAD_POINT, BAD_GAMMA = 3, 300.0      # past the stability edge of RK4 at once
GROUPS = (("pairs", "f64"), ("sp", "f64"), ("sp", "f32"), ("comb", "f64"), ("comb", "f32"))
WIDE = {"f64": 67, "f32": 131}
FIELDS = ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")

# name: (n_steps, save_every, inputs)
SHAPES = {
    "bcast":     (40, 10, "bcast"),      # gamma, alpha, a0: one value for every point
    "lossless":  (40, 1,  "lossless"),   # a broadcast alpha of exactly 0; a0 per point
    "point":     (45, 10, "point"),      # everything per point, one alpha of them 0
    "bad":       (40, 10, "bad"),        # a failing point, exact first_bad_step
    "bad_block": (40, 10, "bad"),        # ... and the save block's last step
}
# (family, precision, shape, N, rows): family "pairs<K>", "sp" or "comb<M>"
_SMALL = ("pairs1", "pairs3", "sp", "comb3", "comb5")
_ROWS = {"lossless": (("sp", "f64"), ("comb3", "f32")),
         "point": (("pairs1", "f64"), ("pairs3", "f64"), ("sp", "f64"), ("sp", "f32"), ("comb5", "f64"), ("comb12", "f64"),
                   ("comb5", "f32"), ("comb12", "f32")),
         "bcast": (("pairs3", "f64"), ("sp", "f64"), ("comb3", "f64"))}
_WIDE = (("pairs1", "f64", "point"), ("sp", "f64", "point"), ("sp", "f32", "point"), ("comb3", "f64", "bad"),
         ("comb5", "f32", "point"))


def group_of(fam: str) -> str:
    return fam.rstrip("0123456789")


def width(fam: str) -> int:
    """Columns of a_end and of the summaries."""
    return 3 if fam == "sp" else (2 + 2 * int(fam[5:]) if fam.startswith("pairs") else int(fam[4:]))


def cases():
    """-> (family, precision, shape name, N, rows)"""
    for fam in _SMALL + ("pairs16", "comb12"):
        for prec in ("f64",) if fam.startswith("pairs") else ("f64", "f32"):
            for name in SHAPES:
                if fam in ("pairs16", "comb12") and name != "point":
                    continue
                if name == "bad_block" and fam.startswith("comb"):   # the comb wrapper has no exact_step: always the exact index
                    continue
                yield fam, prec, name, 5, False
                if (fam, prec) in _ROWS.get(name, ()):
                    yield fam, prec, name, 5, True
    for fam, prec, name in _WIDE:
        yield fam, prec, name, WIDE[prec], False


def inputs(fam: str, N: int, name: str):
    """-> (mismatch, keyword arguments of the family's host wrapper without want_traj)"""
    n_steps, se, kind = SHAPES[name]
    nw = width(fam)
    rng = np.random.default_rng(20250917)
    mis = rng.uniform(-6.0, 2.0, (N_ALL, 16))
    gam = rng.uniform(0.5, 2.0, N_ALL)
    al = rng.uniform(0.5e-2, 3e-2, N_ALL)
    al[1] = 0.0
    strong = rng.uniform(0.2, 0.8, (N_ALL, 34))
    weak = rng.uniform(1e-4, 1e-2, (N_ALL, 34))
    ph = rng.uniform(-3.1, 3.1, (N_ALL, 34))
    if fam.startswith("comb"):        # two strong lines in the middle of the comb
        pw = weak[:, :nw].copy()
        pw[:, nw // 2 - 1:nw // 2 + 1] = strong[:, :2] / 2
        mismatch = mis[:N, :nw]
    elif fam == "sp":                 # [p, s, i]
        pw = np.column_stack([strong[:, 0], weak[:, :2]])
        mismatch = mis[:N, 0]
    else:                             # [p1, p2, s_1, i_1, ...]
        pw = np.column_stack([strong[:, :2] / 2, weak[:, :nw - 2]])
        mismatch = mis[:N, :(nw - 2) // 2]
    a0 = (np.sqrt(pw) * np.exp(1j * ph[:, :nw]))[:N]
    gamma, alpha = 1.1, 1.15e-2
    if kind == "bcast":
        a0 = a0[0]
    elif kind == "lossless":
        alpha = 0.0
    elif kind == "point":
        gamma, alpha = gam[:N], al[:N]
    else:
        gamma = gam[:N].copy()
        gamma[BAD_POINT] = BAD_GAMMA
    kw = dict(n_steps=n_steps, z_max=n_steps * DZ, save_every=se, gamma=gamma, alpha=alpha, a0=np.ascontiguousarray(a0))
    if not fam.startswith("comb"):
        kw["exact_step"] = name != "bad_block"
    return np.ascontiguousarray(mismatch), kw


def _arrays(got: dict) -> dict:
    return {k: v for k, v in got.items() if isinstance(v, np.ndarray)}


def run(nat, fam: str, prec: str, name: str, N: int, rows: bool) -> dict:
    """The host-buffer launch of one case -> its returned arrays (None entries and the time left out)."""
    mismatch, kw = inputs(fam, N, name)
    if fam.startswith("pairs"):
        if not rows:
            return _arrays(nat.sweep_pairs_host(mismatch, **kw))
        one = lambda v: np.asarray(v, float).reshape(1, -1) if np.ndim(v) else np.array([v], float)   # noqa: E731
        kw.update(n_steps=[kw["n_steps"]], seg_len=[kw.pop("z_max")], gamma=one(kw["gamma"]), alpha=one(kw["alpha"]))
        return _arrays(nat.pairs_chain_host(mismatch[None], want_traj=True, **kw))
    if prec == "f32":
        kw["dtype"] = np.float32
    return _arrays((nat.single_pump_host if fam == "sp" else nat.comb_host)(mismatch, want_traj=rows, **kw))


def key(fam, prec, name, N, rows, field) -> str:
    return f"{fam}/{prec}/{name}{'+rows' if rows else ''}/{N}/{field}"


# ---- the `_dev` entry points on torch buffers: 5 points, everything per point, 45 steps saved every tenth ----------------
DEV = (("pairs3", "f64"), ("sp", "f64"), ("sp", "f32"), ("comb5", "f64"), ("comb5", "f32"))


def run_dev(nat, torch, fam: str, prec: str, padded: bool) -> dict:
    """The family's `_dev` entry point on device buffers of the current stream -> the buffers as they come back (SoA).
    padded: with rows and PSA_OPT_TRAJ_LD; for the pairs, whose sweep has no rows, one span of psa_rk4_pairs_chain_f64_dev."""
    N, nw = 5, width(fam)
    mismatch, kw = inputs(fam, N, "point")
    real, cplx = (np.float64, np.complex128) if prec == "f64" else (np.float32, np.complex64)
    tdt = torch.float64 if prec == "f64" else torch.float32
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_mis = t(np.asarray(mismatch, real).T)
    d_g, d_al = t(np.asarray(kw["gamma"], real)), t(np.asarray(kw["alpha"], real))
    d_a0 = t(kw["a0"].astype(cplx).view(real).reshape(N, 2 * nw).T)
    d_aend = torch.empty((2 * nw, N), dtype=tdt, device=dev)
    d_we, d_wm = torch.empty((nw, N), dtype=tdt, device=dev), torch.empty((nw, N), dtype=tdt, device=dev)
    d_bad = torch.empty(N, dtype=torch.int64, device=dev)
    n_steps, se = kw["n_steps"], kw["save_every"]
    ld = nat.traj_ld(N, real)
    d_traj = torch.full((n_steps // se + 1, nw, ld, 2), -7.0, dtype=tdt, device=dev) if padded else None
    flags = nat.OPT_CHECK_NAN | nat.OPT_EXACT_STEP | (nat.OPT_TRAJ_LD if padded else 0)
    grid = dict(stream=torch.cuda.current_stream().cuda_stream, n_points=N, save_every=se, d_gamma=d_g.data_ptr(),
                d_alpha=d_al.data_ptr(), d_a0_soa=d_a0.data_ptr(), flags=flags, d_a_end_soa=d_aend.data_ptr(),
                d_p_wave_end_soa=d_we.data_ptr(), d_p_wave_max_soa=d_wm.data_ptr(), d_first_bad=d_bad.data_ptr())
    traj = dict(d_traj_soa=d_traj.data_ptr()) if padded else {}
    if fam.startswith("pairs"):
        if padded:
            nat.pairs_chain_device(n_pairs=(nw - 2) // 2, n_steps=[n_steps], seg_len=[kw["z_max"]], d_dbeta_soa=d_mis.data_ptr(),
                                   d_transfer_soa=0, **grid, **traj)
        else:
            nat.sweep_pairs_device(n_pairs=(nw - 2) // 2, n_steps=n_steps, z_max=kw["z_max"], d_dbeta_soa=d_mis.data_ptr(), **grid)
    elif fam == "sp":
        nat.single_pump_device(n_steps=n_steps, z_max=kw["z_max"], d_dbeta=d_mis.data_ptr(), dtype=real, **grid, **traj)
    else:
        nat.comb_device(n_lines=nw, n_steps=n_steps, z_max=kw["z_max"], d_kappa_soa=d_mis.data_ptr(), dtype=real, **grid, **traj)
    torch.cuda.synchronize()
    out = dict(a_end=d_aend.cpu().numpy(), p_wave_end=d_we.cpu().numpy(), p_wave_max=d_wm.cpu().numpy(),
               first_bad_step=d_bad.cpu().numpy())
    if padded:
        out["traj"] = d_traj.cpu().numpy()
    return out


def dev_key(fam, prec, padded, field) -> str:
    return f"{fam}/{prec}/{'dev_ld' if padded else 'dev'}/5/{field}"


# ---- one chain of two spans per family that has one besides the single-pump chain of chain_parent_cases.py ----------------
CHAINS = ("pairs3", "comb5")
CHAIN_STEPS = (40, 20)


def run_chain(nat, fam: str) -> dict:
    """(40, 20) steps saved every tenth, a per-point transfer between the spans, rows: 5 points."""
    N, nw = 5, width(fam)
    m0, kw = inputs(fam, N, "point")
    m1, _ = inputs(fam, N, "bcast")
    rng = np.random.default_rng(20250918)
    tr = rng.uniform(0.5, 1.2, (1, N, nw)) * np.exp(1j * rng.uniform(-3.1, 3.1, (1, N, nw)))
    host = nat.pairs_chain_host if fam.startswith("pairs") else nat.comb_chain_host
    return _arrays(host(np.stack([m0, m1[::-1]]), n_steps=list(CHAIN_STEPS), seg_len=[n * DZ for n in CHAIN_STEPS], save_every=10,
                        gamma=np.stack([kw["gamma"], kw["gamma"][::-1]]), alpha=np.array([1.15e-2, 0.0]), a0=kw["a0"],
                        transfers=tr, want_traj=True, exact_step=True))


def chain_key(fam, field) -> str:
    return f"{fam}/f64/chain2/5/{field}"


def expected_keys() -> set:
    want = {key(*c, f) for c in cases() for f in FIELDS + (("traj",) if c[4] else ())}
    want |= {dev_key(fam, prec, padded, f) for fam, prec in DEV for padded in (False, True) for f in FIELDS + (("traj",) if padded else ())}
    return want | {chain_key(fam, f) for fam in CHAINS for f in FIELDS + ("traj",)}
