"""The device dbeta producer (csrc/psa_dbeta.hip; psa_dbeta_grid_* / psa_dbeta_pairs_*) against the exact yardstick of
tests/dbeta_exact.py, on the input sets tests/test_dbeta_exact_host.py holds the host statements to.

Per set (301 points: a block of 256 and a ragged one, rows of 43 changing inside a wave):
  * per point       |device - staged| <= 2 B.  B is the derived first-order bound of the kernel's operation list; the factor 2
                    covers the second-order terms a first-order bound leaves out.
  * end to end      |device - exact(wavelengths)| <= |host scalar - exact(wavelengths)| + 2 B: the triangle inequality through
                    the staged value, which holds only if the device's plan stage is the host's bit for bit.
  * aggregate       median and maximum of e = |device - staged| / scale within FACTOR_MEDIAN, FACTOR_MAX of the host scalar
                    path's (factors measured between the two HOST statements, tests/dbeta_exact.py).  No floor: where only
                    squares enter, the assertion is bit equality with the host.
  * validity        mask and NaN placement equal the host scalar path's.
  * float32         the _f32_dev output is np.float32 of the float64 launch's, bit for bit, NaN and mask in the same places.
  * entry points    psa_dbeta_*_f64 and psa_dbeta_*_f64_dev give the same bits.
Every case prints `dbeta | device | set | median max | twin median max | ratio | worst/B` (record: profiles/dbeta_errors.txt).
"""
from fractions import Fraction

import numpy as np
import pytest

import dbeta_exact as X
import dbeta_hosts as H
import psa_amd._native as nat

pytestmark = pytest.mark.gpu

ALL_CASES = X.CASES + X.CASES_TOLERANCE


def _model(case):
    return nat.dbeta_model(*H.disp_cfg(case))


def _on_device(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def grid_dev(case, l1, ax2, ax3, first=0, n=None, dtype=np.float64):
    """psa_dbeta_grid_{f64,f32}_dev on torch's current stream.  -> (dbeta[n], valid[n])"""
    import torch
    d2, d3 = _on_device(ax2), _on_device(ax3)
    n = d2.numel() * d3.numel() - first if n is None else n
    out = torch.empty(n, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    nat.dbeta_grid_device(_model(case), l1, stream=torch.cuda.current_stream().cuda_stream, d_lambda2_axis=d2.data_ptr(),
                          n2=d2.numel(), d_lambda3_axis=d3.data_ptr(), n3=d3.numel(), first=first, n_points=n,
                          d_dbeta=out.data_ptr(), d_valid=valid.data_ptr(), dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy(), valid.cpu().numpy().astype(bool)


def pairs_dev(model, od, ax1, ax2, first=0, n=None, dtype=np.float64):
    import torch
    d1, d2 = _on_device(ax1), _on_device(ax2)
    n = d1.numel() * d2.numel() - first if n is None else n
    o1, o2 = (torch.empty(n, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda:0") for _ in range(2))
    nat.dbeta_pairs_device(model, od, stream=torch.cuda.current_stream().cuda_stream, d_Omega1_axis=d1.data_ptr(), n1=d1.numel(),
                           d_Omega2_axis=d2.data_ptr(), n2=d2.numel(), first=first, n_points=n, d_dbeta1=o1.data_ptr(),
                           d_dbeta2=o2.data_ptr(), dtype=dtype)
    torch.cuda.synchronize()
    return o1.cpu().numpy(), o2.cpu().numpy()


def same_bits(a, b):
    """Equal element by element as bit patterns, NaN in the same places (a NaN's payload is not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = ~np.isnan(a)
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    return np.array_equal(a[fin].view(bits), b[fin].view(bits))


def is_float64_rounded_once(f32, f64):
    with np.errstate(over="ignore"):
        return f32.dtype == np.float32 and same_bits(f32, f64.astype(np.float32))


def hold_to_the_bars(label, name, got, twin, refs, exact=None):
    """Per point, end to end and aggregate; prints the case's line.  got, twin: the valid points' values."""
    e_got, e_twin = X.unit_errors(got, refs), X.unit_errors(twin, refs)
    worst = X.worst_over_bound(got, refs)
    H.line(label, name, e_got, e_twin, worst)
    for k, (g, r) in enumerate(zip(got, refs)):
        assert abs(Fraction(float(g)) - r[0]) <= 2 * r[2], (name, k, "per point", worst)
    if exact is not None:
        for k, (g, t, r, ex) in enumerate(zip(got, twin, refs, exact)):
            assert abs(Fraction(float(g)) - ex) <= abs(Fraction(float(t)) - ex) + 2 * r[2], (name, k, "end to end")
    assert np.median(e_got) <= X.FACTOR_MEDIAN * np.median(e_twin), (name, "median", np.median(e_got), np.median(e_twin))
    assert e_got.max() <= X.FACTOR_MAX * e_twin.max(), (name, "max", e_got.max(), e_twin.max())


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_grid_kernel_against_the_exact_yardstick(case):
    ev = H.evaluated(case["name"])
    idx = ev["idx"]
    got, ok = nat.dbeta_grid_host(_model(case), X.LAMBDA1, ev["ax2"], ev["ax3"])
    assert got.size == X.N2 * X.N3 == 301
    assert np.array_equal(ok, ev["valid"]) and np.array_equal(np.isnan(got), ~ev["valid"])
    hold_to_the_bars("device", case["name"], got[idx], ev["scalar"][idx], ev["refs"], ev["exact"])
    if case["name"] in X.ORDERS_LE_2:
        assert same_bits(got, ev["scalar"])
    dev, ok_dev = grid_dev(case, X.LAMBDA1, ev["ax2"], ev["ax3"])
    assert same_bits(dev, got) and np.array_equal(ok_dev, ok)
    f32, ok32 = grid_dev(case, X.LAMBDA1, ev["ax2"], ev["ax3"], dtype=np.float32)
    assert is_float64_rounded_once(f32, got) and np.array_equal(ok32, ok)


@pytest.mark.parametrize("orders", X.PAIR_ORDER_SETS, ids=str)
def test_pairs_kernel_against_the_exact_yardstick(orders):
    """Two Omega axes with negative entries and Omega = 0: point i gets (dbeta(Omega1[i // n2]), dbeta(Omega2[i % n2]))."""
    ev = H.evaluated_pairs(orders)
    a1, a2 = ev["axis1"], ev["axis2"]
    model = nat.dbeta_model(H.disp_cfg(ev["case"])[0], None, even_orders=orders)
    g1, g2 = nat.dbeta_pairs_host(model, ev["od"], a1["axis"], a2["axis"])
    rows, cols = np.divmod(np.arange(X.N2 * X.N3), X.N3)
    assert g1.size == 301 and (a1["axis"] == 0).any() and (a2["axis"] == 0).any() and (a1["axis"] < 0).any() and (a2["axis"] < 0).any()
    hold_to_the_bars("device", f"pairs {orders} axis 1", g1, a1["scalar"][rows], [a1["refs"][r] for r in rows])
    hold_to_the_bars("device", f"pairs {orders} axis 2", g2, a2["scalar"][cols], [a2["refs"][c] for c in cols])
    d1, d2 = pairs_dev(model, ev["od"], a1["axis"], a2["axis"])
    assert same_bits(d1, g1) and same_bits(d2, g2)
    f1, f2 = pairs_dev(model, ev["od"], a1["axis"], a2["axis"], dtype=np.float32)
    assert is_float64_rounded_once(f1, g1) and is_float64_rounded_once(f2, g2)
    e1, e2 = nat.dbeta_pairs_host(model, ev["od"], a1["axis"], a2["axis"], first=37, n_points=250)
    assert same_bits(e1, g1[37:287]) and same_bits(e2, g2[37:287])


def test_every_validity_rule_on_the_device():
    """The rule-by-rule points of tests/test_dbeta_exact_host.py (each invalid on the scalar path for its own reason, shown
    there): invalid and NaN on the device, in float64 and float32; valid under the neighbouring case where one is given."""
    for label, case, l1, l2, l3, _, valid_under in X.rule_points():
        assert not H.scalar_point(case, l1, l2, l3)[1]
        got, ok = nat.dbeta_grid_host(_model(case), l1, [l2], [l3])
        assert not ok[0] and np.isnan(got[0]), (label, case["name"])
        f32, ok32 = grid_dev(case, l1, [l2], [l3], dtype=np.float32)
        assert not ok32[0] and np.isnan(f32[0]), (label, case["name"])
        if valid_under is not None:
            want = H.scalar_point(valid_under, l1, l2, l3)
            got, ok = nat.dbeta_grid_host(_model(valid_under), l1, [l2], [l3])
            assert want[1] and ok[0] and np.isfinite(got[0]), (label, valid_under["name"])


@pytest.mark.parametrize("case", [X.CASE_SYM, X.CASE_TAYLOR], ids=["symmetric", "taylor"])
def test_wide_grid_mask_equals_the_scalar_paths(case):
    """A 64 x 64 cut of the wide grid of tools/dbeta_fuzz.py, specials included.  The shares are checked on the host path alone,
    so the comparison cannot pass on an empty mask."""
    l2, l3 = X.wide_axes()
    want, valid, _ = H.scalar_grid(case, X.LAMBDA1, X.grid_points(l2, l3))
    assert (~valid).mean() >= 0.1 and valid.mean() >= 1 / 3
    got, ok = nat.dbeta_grid_host(_model(case), X.LAMBDA1, l2, l3)
    assert np.array_equal(ok, valid) and np.array_equal(np.isnan(got), ~valid)
    f32, ok32 = grid_dev(case, X.LAMBDA1, l2, l3, dtype=np.float32)
    assert np.array_equal(ok32, valid) and is_float64_rounded_once(f32, got)


@pytest.mark.parametrize("first", X.BIG_FIRSTS, ids=["across 2^31", "across 2^32", "row boundary above 2^32"])
def test_blocks_of_a_grid_of_4_9e9_points(first):
    """70 001 x 70 001 points, of which only the axes travel: 300 points at `first` from the host entry, the _dev entry, the
    float32 entry and the pairs kernel are the same bits as the launch on the grid made of the block's rows alone, whose indices
    are small; rows and first index of that grid come from Python integers."""
    n = X.BIG_POINTS
    rows, first_small = X.small_grid_of(first, n, X.BIG_N)
    assert [first // X.BIG_N, (first + n - 1) // X.BIG_N] == [rows[0], rows[-1]]
    ax2, ax3 = X.big_axes()
    for case in (X.CASE_SYM, X.CASE_TAYLOR):
        model = _model(case)
        want, ok_want = nat.dbeta_grid_host(model, X.LAMBDA1, ax2[rows], ax3, first=first_small, n_points=n)
        pairs = [(ax2[(first + t) // X.BIG_N], ax3[(first + t) % X.BIG_N]) for t in (0, n - 1)]
        for t, (l2, l3) in zip((0, n - 1), pairs):                                # the ends of the block, one point at a time
            assert same_bits(nat.dbeta_grid_host(model, X.LAMBDA1, [l2], [l3])[0], want[t:t + 1])
        assert ok_want.all() and np.unique(want).size == n
        got, ok = nat.dbeta_grid_host(model, X.LAMBDA1, ax2, ax3, first=first, n_points=n)
        assert same_bits(got, want) and ok.all(), (case["name"], "host entry")
        got, ok = grid_dev(case, X.LAMBDA1, ax2, ax3, first, n)
        assert same_bits(got, want) and ok.all(), (case["name"], "_dev entry")
        f32, ok = grid_dev(case, X.LAMBDA1, ax2, ax3, first, n, dtype=np.float32)
        assert is_float64_rounded_once(f32, want) and ok.all(), (case["name"], "_f32_dev entry")
    o1, o2 = X.big_pair_axes()
    model = nat.dbeta_model(H.disp_cfg(X.CASE_SYM)[0], None, even_orders=(2, 4))
    w1, w2 = nat.dbeta_pairs_host(model, X.PAIR_OMEGA_D, o1[rows], o2, first=first_small, n_points=n)
    assert np.unique(w2).size == n
    g1, g2 = nat.dbeta_pairs_host(model, X.PAIR_OMEGA_D, o1, o2, first=first, n_points=n)
    assert same_bits(g1, w1) and same_bits(g2, w2)
    d1, d2 = pairs_dev(model, X.PAIR_OMEGA_D, o1, o2, first, n)
    assert same_bits(d1, w1) and same_bits(d2, w2)
    f1, f2 = pairs_dev(model, X.PAIR_OMEGA_D, o1, o2, first, n, dtype=np.float32)
    assert is_float64_rounded_once(f1, w1) and is_float64_rounded_once(f2, w2)
