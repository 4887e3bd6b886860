"""The gain summary (gain_pass1 / gain_pass2 in csrc/psa_aux.hip) at its edges: ties at every merge level, the grid-stride loop
behind the 2 048-block cap, the second pass over 2 048 partials, and the float32 variant.

Reference: NumPy in float64.  gain = p / p0, or 10 log10 of it; a point is valid where p and the gain are finite, the gain is
positive and first_bad_step < 0.  best_index = np.argmax over the valid gains -- the FIRST maximum --, n_finite their count.

Layout the tie cases rely on (gain_blocks, gain_pass1): for N <= 2 048 * 256 block b holds points [256 b, 256 b + 256), thread t
of it point 256 b + t, in wave t // 64 and lane t % 64; beyond that 2 048 blocks stride by 2 048 * 256 = 524 288.  gain_pass2 is
one block of 256 threads; thread t folds partials t, t + 256, ...
"""
import numpy as np
import pytest

import psa_amd._native as nat

pytestmark = pytest.mark.gpu

P0 = 3e-7                                  # not a power of two: p / p0 rounds
STRIDE = 2048 * 256
N_BIG = STRIDE + 77


def reference(p, bad, p0, db):
    """-> (gain[N] float64 with NaN, best_index, best_gain, n_finite)"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = p / p0
        ok = np.isfinite(p) & np.isfinite(g) & (g > 0)
        if bad is not None:
            ok &= np.asarray(bad) < 0
        gain = np.where(ok, 10.0 * np.log10(np.where(ok, g, 1.0)) if db else g, np.nan)
    if not ok.any():
        return gain, -1, float("nan"), 0
    best = int(np.argmax(np.where(ok, gain, -np.inf)))
    return gain, best, float(gain[best]), int(ok.sum())


def check(p, bad, p0=P0, db=True, want_index=None):
    """One launch against the reference.  Linear gain: bit-equal (one IEEE division; float32: that quotient rounded once).
    dB, float64: rtol 1e-14, the bar of test_gain_summary_reduction_matches_numpy.  dB, float32: gain_out is the float64 gain
    rounded once -- np.float32 of 10 * L with L NumPy's log10 or one of its two float64 neighbours, log10 being held to one
    float64 ulp BEFORE the rounding.  best_gain is the float64 value in both variants."""
    gain, bi, bg, nf = nat.gain_summary_host(p, bad, p0, gain_db=db)
    ref, r_bi, r_bg, r_nf = reference(p, bad, p0, db)
    f32 = np.asarray(p).dtype == np.float32
    assert gain.dtype == (np.float32 if f32 else np.float64)
    assert np.array_equal(np.isnan(gain), np.isnan(ref))
    fin = ~np.isnan(ref)
    if not db:
        assert np.array_equal(gain[fin], ref[fin].astype(gain.dtype))
    elif f32:
        L = np.log10(np.asarray(p, dtype=np.float64)[fin] / p0)
        near = [(10.0 * x).astype(np.float32) for x in (np.nextafter(L, -np.inf), L, np.nextafter(L, np.inf))]
        assert np.all((gain[fin] == near[0]) | (gain[fin] == near[1]) | (gain[fin] == near[2]))
    else:
        np.testing.assert_allclose(gain[fin], ref[fin], rtol=1e-14, atol=0)
    assert nf == r_nf and bi == r_bi, (bi, r_bi, nf, r_nf)
    if want_index is not None:
        assert bi == want_index
    if r_bi < 0:
        assert np.isnan(bg)
    else:
        assert bg == (pytest.approx(r_bg, rel=1e-14) if db else r_bg)
    return gain, bi, bg, nf


def background(n, dtype, seed=11):
    """Distinct powers well below the planted maximum, with a few invalid points of every kind."""
    rng = np.random.default_rng(seed)
    p = (10 ** rng.uniform(-9, -4, n)).astype(dtype)
    bad = np.full(n, -1, np.int64)
    k = max(1, n // 60)
    p[rng.integers(0, n, k)] = np.nan
    p[rng.integers(0, n, k)] = np.inf
    p[rng.integers(0, n, k)] = 0.0
    p[rng.integers(0, n, k)] = -1e-5
    bad[rng.integers(0, n, k)] = 3
    return p, bad


# (name, N, lower index, higher index): the tied pair straddles one merge level
TIES = [
    ("two lanes of a wave, xor 1", 300, 256 + 4, 256 + 5),
    ("two lanes of a wave, xor 32", 300, 3, 35),
    ("two lanes of a wave, xor 63", 300, 64, 127),
    ("two waves of a block", 300, 10, 64 + 10),
    ("waves 1 and 3 of a block", 1100, 256 + 70, 256 + 200),
    ("two blocks", 1100, 100, 256 * 3 + 7),
    ("the ragged last block", 1100, 1, 1099),
    ("two partials in one wave of the second pass", 70_001, 256 * 2 + 9, 256 * 40 + 200),
    ("two partials in different waves of the second pass", 70_001, 256 * 3 + 1, 256 * 70 + 2),
    ("two partials of one thread of the second pass", 70_001, 256 * 2 + 9, 256 * 258 + 9),
    ("one thread's two grid-stride trips", N_BIG, 5, STRIDE + 5),
    ("grid stride: last thread with a second trip against its first", N_BIG, 76, STRIDE + 76),
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,n,lo,hi", TIES, ids=[t[0] for t in TIES])
def test_a_tie_goes_to_the_lower_index(name, n, lo, hi, dtype):
    """The maximum planted at two indices.  "Both memory orders": the pair at (lo, hi), and the mirrored pair at
    (n - 1 - hi, n - 1 - lo), which swaps the two operands' places in every merge; and a third copy beyond the pair, which must
    not win either.  dB and linear."""
    p, bad = background(n, dtype)
    top = dtype(2.5e-3)
    for a, b in ((lo, hi), (n - 1 - hi, n - 1 - lo)):
        q, qbad = p.copy(), bad.copy()
        q[[a, b]] = top
        qbad[[a, b]] = -1
        for db in (True, False):
            check(q, qbad, db=db, want_index=a)
        if b + 1 < n:
            q[n - 1], qbad[n - 1] = top, -1
            check(q, qbad, want_index=a)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 64, 300, 70_001, N_BIG])
def test_all_gains_equal_gives_index_zero_and_a_lone_valid_last_point_wins(n, dtype):
    p = np.full(n, 4.25e-4, dtype)
    for db in (True, False):
        gain, bi, bg, nf = check(p, None, db=db, want_index=0)
        assert nf == n
    p = np.full(n, np.nan, dtype)
    p[n - 1] = 1e-5
    gain, bi, bg, nf = check(p, np.full(n, -1, np.int64), want_index=n - 1)
    assert nf == 1
    bad = np.full(n, 5, np.int64)                # ... and with first_bad_step deciding instead of the power
    bad[n - 1] = -1
    gain, bi, bg, nf = check(np.full(n, 4.25e-4, dtype), bad, want_index=n - 1)
    assert nf == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_grid_stride_and_the_second_pass_over_2048_partials(dtype):
    """N = 2 048 * 256 + 77: every block's first 77 threads make two trips, gain_pass2 folds 2 048 partials, eight per thread."""
    assert nat.gain_summary_workspace_bytes(N_BIG) == nat.gain_summary_workspace_bytes(STRIDE) == 2048 * 24
    p, bad = background(N_BIG, dtype)
    top = dtype(2.5e-3)
    q = p.copy()
    q[STRIDE + 40], bad[STRIDE + 40] = top, -1            # the maximum in the tail beyond 2 048 * 256
    gain, bi, bg, nf = check(q, bad, want_index=STRIDE + 40)
    assert nf == reference(q, bad, P0, True)[3] and 0.9 * N_BIG < nf < N_BIG
    q = p.copy()
    q[0] = q[STRIDE + 60] = top                           # at index 0, with a tie in the tail
    bad[[0, STRIDE + 60]] = -1
    check(q, bad, want_index=0)
    check(q, bad, db=False, want_index=0)
    q[0] = dtype(1e-6)                                    # the last point of all, alone at the top
    q[N_BIG - 1], bad[N_BIG - 1] = dtype(5e-3), -1
    check(q, bad, want_index=N_BIG - 1)


def test_float32_best_index_follows_the_float64_gains():
    """Two float32 powers one ulp apart at ~40 dB: their float64 gains differ, the float32 gains written out are the same
    number.  The larger float64 gain wins wherever it stands -- also at the higher index, where a comparison of the rounded
    gains would keep the lower."""
    lo = np.float32(3e-3)
    hi = np.nextafter(lo, np.float32(1))
    ref, *_ = reference(np.array([lo, hi]), None, P0, True)
    assert ref[1] > ref[0] and np.float32(ref[0]) == np.float32(ref[1])          # the condition on the inputs
    for n, i, j in ((300, 7, 200), (300, 64 + 3, 64 + 4), (70_001, 256 * 3 + 1, 256 * 70 + 2), (N_BIG, 5, STRIDE + 5)):
        p, bad = background(n, np.float32)
        bad[[i, j]] = -1
        for a, b in ((i, j), (j, i)):                     # the larger one at the higher index, then at the lower
            p[a], p[b] = lo, hi
            gain, bi, bg, nf = check(p, bad, want_index=b)
            assert gain[a] == gain[b] and bg == pytest.approx(ref[1], rel=1e-14) and bg != float(gain[b])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_no_first_bad_array_is_an_array_of_minus_one(dtype):
    for n in (300, 70_001):
        p, _ = background(n, dtype)
        for db in (True, False):
            a = check(p, None, db=db)
            b = check(p, np.full(n, -1, np.int64), db=db)
            assert np.array_equal(a[0], b[0], equal_nan=True) and a[1:] == b[1:]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("p0", [0.0, -0.0, -1e-7, float("nan"), float("inf")])
def test_a_seed_power_that_is_no_power_makes_everything_nan(p0, dtype):
    """p0 zero, negative or NaN (and infinite: every gain 0, not positive): all gains NaN, index -1, count 0."""
    p = (10 ** np.random.default_rng(4).uniform(-9, -2, 1100)).astype(dtype)
    for db in (True, False):
        gain, bi, bg, nf = check(p, None, p0=p0, db=db)
        assert np.isnan(gain).all() and bi == -1 and nf == 0 and np.isnan(bg)
