"""The cases of tests/test_gpu_chain_parent.py, shared with gen_golden_chain_parent.py (which records chain_parent.npz).

Host-buffer chains of both families (nat.chain_host: 4 and 6 waves, float64 and float32; nat.single_pump_chain_host), the
smallest that reach every line the two families share from the C entry points up: N = 5 (less than one wave) and 67 (a
partial second wave); S = 1, 2, 3 spans of (40), (40, 20), (20, 40, 10) steps; save_every 1 and 10; no, broadcast and
per-point transfers; gamma and alpha one value per span or per point in one span; a lossless middle span between lossy
ones; with and without the per-wave summary and the trajectory (the 4/6-wave summary takes no trajectory); and a point that
goes non-finite in the second span.  Every launch draws its inputs from the same 67 points."""
import numpy as np

N_ALL = 67
STEPS = {1: (40,), 2: (40, 20), 3: (20, 40, 10)}
DZ = 0.1
FAMILIES = (("w4", "f64"), ("w6", "f64"), ("sp", "f64"), ("w4", "f32"), ("w6", "f32"))
WIDTH = {"w4": 4, "w6": 6, "sp": 3}
BAD_POINT, BAD_GAMMA = 3, 300.0      # past the stability edge of RK4 at once: the span's first step fails

# name: (S, save_every, transfers, per-point gamma/alpha span or None, alpha of the spans, summary, trajectory, failing)
SHAPES = {
    "one":       (1, 10, None,    None, (1.15e-2,),            False, False, False),
    "one_rows":  (1, 1,  None,    0,    (1.15e-2,),            False, True,  False),
    "one_wsum":  (1, 1,  None,    None, (0.0,),                True,  False, False),
    "two_bcast": (2, 1,  "bcast", 1,    (1.15e-2, 2e-2),       False, True,  False),
    "two_point": (2, 10, "point", None, (1.15e-2, 0.0),        True,  False, False),
    "two_rows":  (2, 10, "point", 0,    (1.15e-2, 2e-2),       False, True,  False),
    "three":     (3, 10, "point", 2,    (1.15e-2, 0.0, 2e-2),  True,  False, False),
    "three_mid": (3, 10, "bcast", None, (1.15e-2, 0.0, 2e-2),  False, True,  False),
    "three_all": (3, 1,  None,    None, (0.0, 0.0, 0.0),       True,  False, False),
    "three_row": (3, 1,  "point", 1,    (1.15e-2, 0.0, 2e-2),  False, True,  False),
    "bad":       (2, 10, "bcast", None, (1.15e-2, 0.0),        False, False, True),
    "bad_wsum":  (3, 10, "point", None, (1.15e-2, 1e-2, 0.0),  True,  False, True),
}
# (shape, N) per family: the long rows stay at 5 points, and the 67-point launches are spread over the families (the record
# stays small)
WIDE = {("w4", "f64"): ("one", "three", "bad"), ("w6", "f64"): ("two_point",), ("sp", "f64"): ("three", "bad_wsum"),
        ("w4", "f32"): ("one", "two_rows"), ("w6", "f32"): ("three", "bad")}
ROWS_AT_5 = {("w4", "f64"): ("one_rows", "three_mid"), ("w6", "f64"): ("two_rows", "three_mid"), ("sp", "f64"): ("three_row", "three_mid"),
             ("w4", "f32"): ("two_bcast", "three_mid"), ("w6", "f32"): ("one_rows", "two_rows")}
FIELDS = {"w4": ("a_end", "p_end", "p_max", "first_bad_step"), "sp": ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")}
FIELDS["w6"] = FIELDS["w4"]


def cases():
    """-> (family, precision, shape name, N)"""
    for fam, prec in FAMILIES:
        for name, shape in SHAPES.items():
            if shape[6]:
                sizes = ((5,) if name in ROWS_AT_5[fam, prec] else ()) + ((67,) if name in WIDE[fam, prec] else ())
            else:
                sizes = (5,) + ((67,) if name in WIDE[fam, prec] else ())
            for N in sizes:
                yield fam, prec, name, N


def inputs(fam: str, N: int, shape):
    S, se, transfers, per_point, alphas, wsum, traj, failing = shape
    nw = WIDTH[fam]
    rng = np.random.default_rng(20250311)
    db = rng.uniform(-6.0, 2.0, (3, N_ALL))
    db2 = rng.uniform(-6.0, 2.0, (3, N_ALL))
    gam = rng.uniform(0.5, 2.0, (3, N_ALL))
    al = rng.uniform(0.5e-2, 3e-2, N_ALL)
    pw = rng.uniform([0.2] * 2 + [1e-4] * 4, [0.8] * 2 + [1e-2] * 4, (N_ALL, 6))
    ph = rng.uniform(-3.1, 3.1, (N_ALL, 6))
    tg = rng.uniform(0.5, 1.2, (2, N_ALL, 6)) * np.exp(1j * rng.uniform(-3.1, 3.1, (2, N_ALL, 6)))
    a0 = np.sqrt(pw) * np.exp(1j * ph)
    cols = slice(1, 4) if fam == "sp" else slice(0, nw)       # [p, s, i] or [p1, p2, s, i, ...]
    gamma = np.array([1.1, 0.7, 1.6][:S])
    alpha = np.array(alphas, float)
    if per_point is not None:                                  # one span per point makes the whole array (S, N)
        gamma = np.repeat(gamma[:, None], N, axis=1)
        gamma[per_point] = gam[per_point, :N]
        alpha = np.repeat(alpha[:, None], N, axis=1)
        if alphas[per_point] != 0.0:
            alpha[per_point] = al[:N]
    if failing:
        gamma = np.repeat(gamma[:, None], N, axis=1) if gamma.ndim == 1 else gamma
        gamma[1, BAD_POINT] = BAD_GAMMA
    tr = None
    if transfers == "bcast":
        tr = np.ascontiguousarray(tg[:S - 1, 0, cols])
    elif transfers == "point":
        tr = np.ascontiguousarray(tg[:S - 1, :N, cols])
    kw = dict(n_steps=list(STEPS[S]), seg_len=[n * DZ for n in STEPS[S]], save_every=se, gamma=gamma, alpha=alpha,
              a0=np.ascontiguousarray(a0[:N, cols]), transfers=tr, want_traj=traj, exact_step=True)
    if fam == "w6":
        kw["dbeta2"] = np.ascontiguousarray(db2[:S, :N])
    return np.ascontiguousarray(db[:S, :N]), kw


def run(nat, fam: str, prec: str, name: str, N: int) -> dict:
    """The launch of one case -> its returned arrays (None entries and the time left out)."""
    shape = SHAPES[name]
    db, kw = inputs(fam, N, shape)
    if fam == "sp":
        got = nat.single_pump_chain_host(db, **kw)
    else:
        got = nat.chain_host(db, dtype=np.float64 if prec == "f64" else np.float32, wave_summary=shape[5], **kw)
    return {k: v for k, v in got.items() if isinstance(v, np.ndarray)}


def expected_fields(fam: str, name: str):
    shape = SHAPES[name]
    f = FIELDS[fam] + (("p_wave_end", "p_wave_max") if shape[5] and fam != "sp" else ())
    return f + (("traj",) if shape[6] else ())


def key(fam, prec, name, N, field) -> str:
    return f"{fam}/{prec}/{name}/{N}/{field}"


def pack(records: dict) -> dict:
    """One byte string for all arrays (an archive member per array would outweigh the small ones) and one index line
    "key|dtype|shape|offset" per array; arrays that repeat share their bytes."""
    blob, index, seen = bytearray(), [], {}
    for k, a in records.items():
        raw = np.ascontiguousarray(a).tobytes()
        if raw not in seen:
            seen[raw] = len(blob)
            blob += raw
        index.append(f"{k}|{a.dtype.str}|{','.join(map(str, a.shape))}|{seen[raw]}")
    return dict(blob=np.frombuffer(bytes(blob), np.uint8), index=np.array(index))


def unpack(npz) -> dict:
    blob, out = npz["blob"].tobytes(), {}
    for line in npz["index"]:
        k, dt, shape, off = str(line).split("|")
        shape = tuple(int(x) for x in shape.split(","))
        out[k] = np.frombuffer(blob, np.dtype(dt), int(np.prod(shape)), int(off)).reshape(shape)
    return out
