"""The case grid of tests/test_gpu_row_loop.py, shared with gen_golden_row_loop.py (which records row_loop_parent.npz).

Summary launches (no trajectory) of the fused float64 4-wave one-lane kernel: the instantiations whose z-loop runs by saved
rows.  Points: 131 with per-point dbeta, gamma and amplitudes (phases included), `mirrored` (A2 == A1 and A4 == A3 bit for
bit: the mirrored loop) or `asym` (one lane of every wave with unequal pumps: the whole wave takes the general loop); a
launch of N = 67 takes the first 67 of them (two waves, the second partial), so its record is the first 67 rows of the
131-point one -- points do not interact."""
import numpy as np

N_ALL = 131
SIZES = (67, 131)
SETS = ("mirrored", "asym")
ASYM_LANES = (5, 65, 129)            # one per wave of 64; 5 and 65 are inside N = 67
# (n_steps, save_every): no row | every remainder 0..3 of the 4-step trip, tails of 0..3 and more steps, several rows per
# test group | one row per group (save_every = 64) and groups longer than 64 steps
STEPS = ((5, 7), (9, 1), (11, 2), (10, 3), (8, 4), (23, 5), (64, 7), (205, 10), (200, 64), (131, 65), (250, 100))
CHECKS = ("off", "block", "exact")
LOSSY = (True, False)
LAYOUTS = ((False, 64), (False, 256), (True, 256))    # (per-wave summary, threads per workgroup): the summary has 256 only
FIELDS = ("a_end", "p_end", "p_max", "first_bad_step")
WAVE_FIELDS = ("p_wave_end", "p_wave_max")
DZ = 0.1


def points(which: str):
    """-> dbeta (131,), gamma (131,), a0 (131, 4) complex"""
    rng = np.random.default_rng(20240607)
    db = rng.uniform(-6.0, 2.0, N_ALL)
    gam = rng.uniform(0.5, 2.0, N_ALL)
    pw = rng.uniform([0.2, 1e-4], [0.8, 1e-2], (N_ALL, 2))
    ph = rng.uniform(-3.1, 3.1, (N_ALL, 2))
    half = np.sqrt(pw) * np.exp(1j * ph)
    a0 = np.stack([half[:, 0], half[:, 0], half[:, 1], half[:, 1]], axis=1)
    if which == "asym":
        for lane in ASYM_LANES:
            a0[lane, 1] *= 0.9
            a0[lane, 3] *= np.exp(0.3j)
    elif which != "mirrored":
        raise ValueError(which)
    return db, gam, np.ascontiguousarray(a0)


def check_kw(check: str) -> dict:
    return dict(check_nan=check != "off", exact_step=(check == "exact") if check != "off" else None)


def run(nat, which: str, N: int, n_steps: int, se: int, check: str, lossy: bool, wsum: bool = False, block: int = 256,
        traj: bool = False) -> dict:
    """One one-lane launch of the case; a scalar alpha of 0 selects the lossless instantiation."""
    db, gam, a0 = points(which)
    flags = nat.OPT_ONE_LANE | (nat.OPT_BLOCK64 if block == 64 else 0)
    return nat.sweep_host(db[:N], n_steps=n_steps, z_max=n_steps * DZ, save_every=se, gamma=gam[:N],
                          alpha=1.15e-2 if lossy else 0.0, a0=a0[:N], extra_flags=flags, wave_summary=wsum, want_traj=traj,
                          **check_kw(check))


def key(which, n_steps, se, check, lossy, wsum, block, field) -> str:
    return f"{which}/{n_steps}x{se}/{check}/{'lossy' if lossy else 'lossless'}/{'wsum' if wsum else 'plain'}{block}/{field}"


def variants():
    for check in CHECKS:
        for lossy in LOSSY:
            for wsum, block in LAYOUTS:
                yield check, lossy, wsum, block


def pack(records: dict) -> dict:
    """Arrays that repeat (the check mode, the workgroup size and the per-wave summary change no bit of the others) are
    stored once; `alias` lists "key=stored key" for the rest."""
    store, alias, seen = {}, [], {}
    for k, a in records.items():
        sig = (a.dtype.str, a.shape, a.tobytes())
        if sig in seen:
            alias.append(f"{k}={seen[sig]}")
        else:
            seen[sig] = k
            store[k] = a
    store["alias"] = np.array(alias)
    return store


def unpack(npz) -> dict:
    out = {k: npz[k] for k in npz.files if k != "alias"}
    for line in npz["alias"]:
        k, v = str(line).split("=")
        out[k] = out[v]
    return out
