"""Every sweep kernel against the 80-bit RK4 yardstick (tests/truth_ld.py), through the C-ABI host entries of _native.

The other GPU parity tests hold a kernel within RTOL_F64 = 1e-9 of a float64 twin while the kernels sit at 1e-12..1e-13 of
theirs: three decimal digits in which a kernel can get worse unseen, and no way to say whose error a disagreement is.  Here
kernel and twin are both measured against the same discrete scheme run 2 000 times finer than float64, and the bar is "no
worse than a plain float64 RK4 by more than a stated factor":

    median(e_gpu) <= max(4 median(e_twin), floor)   and   max(e_gpu) <= max(8 max(e_twin), floor)

over the N points, e = point_err against the yardstick, on a_end, on the power summaries and on the rows where a case has
them.  The factors are about three times the spread between two plain float64 statements of the scheme (medians within 1.3x,
maxima within 2.4x of each other: tests/test_truth_host.py measures it); the floor 2e-14 is the drift budget psa_rk4_kernel.inc.h states
for the carried phase (1.4e-14) plus rounding, 2e-6 the same budget in float32 against a plain float32 RK4.  Neither comes
from a kernel's own figures.  The RTOL_F64 / RTOL_F32 assertion against the twin is kept alongside.

Where a documented design choice makes an output miss the bar, the strict xfail expects BarMissed for that output alone: the
other outputs, the twin at RTOL_F64, first_bad_step and a band -- the bar plus the drift the kernel's header states for the
choice -- are asserted as in every other case, and failing any of them fails the test.

The cases at 100 000 steps (float64) and at 1e5 / 1e6 steps (float32) take yardstick and twins from a compiled plain RK4
(oracle/plain_rk4.py, pinned in tests/test_truth_long_host.py); float32 has a second bar there, against a compensated float32
twin of the kernel's kind, with no floor.

Inputs, shapes and the cached 80-bit runs: tests/truth_cases.py.  Each case prints one line of the record
(profiles/truth_errors.txt)."""
import functools

import numpy as np
import pytest

import truth_cases as TC
import truth_ld as T
from conftest import RTOL_F32, RTOL_F64

import psa_amd._native as nat

pytestmark = pytest.mark.gpu


class BarMissed(AssertionError):
    """An output misses the bar.  The strict xfails below expect this and nothing else: every other assertion of such a case
    -- first_bad_step, the twin at RTOL_F64, the outputs that are not known to miss, the band on those that are -- fails it."""


def check(family, case, got, inputs, floor=TC.FLOOR_F64, rtol=RTOL_F64, known=(), budget=0.0):
    """Every assertion of a case but the last.  ``known``: the outputs a documented design choice lets miss the bar; each of
    them stays within the bar plus ``budget``, the drift the kernel's header states for that choice (never a figure measured
    on the kernel).  -> the outputs that miss the bar; the caller raises BarMissed for them."""
    assert (got["first_bad_step"] == -1).all()
    missed = TC.judge(family, case, got, inputs, floor)
    # the bar of record: against the float64 twin, and in float32 (whose twin is no reference) against the yardstick
    for key, e in TC.errors(got, inputs["twin" if rtol == RTOL_F64 else "truth"]).items():
        assert e.max() < rtol, (key, e.max())
    assert set(missed) <= set(known), "\n".join(missed[k][0] for k in missed if k not in known)
    for key, (line, med, mx, tmed, tmx) in missed.items():
        b_med, b_max = budget[key] if isinstance(budget, dict) else (budget, budget)   # one budget, or (median, max) per output
        assert med <= max(4.0 * tmed, floor) + b_med and mx <= max(8.0 * tmx, floor) + b_max, f"beyond the stated drift: {line}"
    return missed


def meets_the_bar(missed):
    if missed:
        raise BarMissed("\n".join(line for line, *_ in missed.values()))


def sweep_kw(inputs):
    return {k: inputs[k] for k in ("n_steps", "z_max", "save_every", "gamma", "alpha", "a0")}


# ---- findings at HEAD: strict xfails on BarMissed alone, each a consequence of a documented design choice -----
R_OFF_UNIT = 5.5e-17      # psa_rk4_kernel.inc.h: "the modulus of the rounded r, <= 5.5e-17 off one, now accumulates in the sidebands"
CARRIED_BUDGET = 1.4e-14  # psa_rk4_kernel.inc.h: "drift <= 128 multiplications ~1.4e-14" between two seeds of a carried factor
FRAME_DRIFT = (
    "the one-lane float64 4-wave step is frame-anchored (psa_rk4_kernel.inc.h, rk4_step_on): after every step the sidebands are "
    "multiplied by the rounded r = exp(i dbeta h/2), and |r| - 1 is a lane constant of ONE sign, up to 5.5e-17, so the sidebands' "
    "moduli drift by n (|r| - 1) -- up to 8e-14 of themselves after 1 500 steps, 5.5e-13 after 10 000 -- where a plain RK4's "
    "random-walk.  The kernel header states the choice (5.5e-12 of the sidebands after 1e5 steps, for 10 instructions per step).  This mark stands "
    "in for a fix that has not been made.  Measured: ")
CARRIED_U = (
    "the comb kernel carries u_m = exp(i kappa_m z) by two rotations per step between exact seeds 64 steps apart "
    "(psa_rk4_comb_kernel.inc.h): up to 128 roundings of one sign in |u_m| and in its angle, the 1.4e-14 drift budget "
    "psa_rk4_kernel.inc.h states, on every line -- the pumps included from M = 4 on.  Every case with M >= 4 has an a_end median "
    "3.9x..6.3x the twin's (1.5e-14..2.3e-14), AT the 2e-14 floor: which of them land above it is a matter of 1-2 %, so the "
    "family is one finding with one mark.  This mark stands in for a fix that has not been made.")


def xfail(why, figures=""):
    return pytest.mark.xfail(strict=True, raises=BarMissed, reason=why + figures)


# ---- four waves, float64 ---------------------------------------------------------------------------------------------------
LAYOUTS = dict(one_lane=nat.OPT_ONE_LANE, split=nat.OPT_SPLIT_POINT, quad=nat.OPT_QUAD_POINT, lds=nat.OPT_LDS_STAGING)
SIGNAL_POWER = ("p_end", "p_max")     # what the frame's drift moves at 1 500 steps: a_end, scaled to the pumps, stays inside the bar
WAVES4 = [
    pytest.param("one_lane", False, True, marks=xfail(FRAME_DRIFT, "p_end median 8.5e-16 (33x the twin's), max 3.1e-14 (24x)")),
    ("one_lane", False, False),
    pytest.param("one_lane", True, True, marks=xfail(FRAME_DRIFT, "p_end median 2.1e-16 (17x the twin's), max 4.8e-14 (31x)")),
    pytest.param("one_lane", True, False, marks=xfail(FRAME_DRIFT, "p_end median 4.6e-16 (21x the twin's), max 2.5e-14 (17x)")),
    ("split", False, True), ("split", False, False), ("quad", False, True), ("quad", False, False), ("lds", False, True)]


@pytest.mark.parametrize("layout,mirrored,lossy", WAVES4)
def test_four_waves(layout, mirrored, lossy):
    """In the one-lane layout the signal's power may miss the bar by the frame's stated drift, n (|r| - 1), and no more; a_end,
    the twin at RTOL_F64 and first_bad_step hold in every case, xfailed or not."""
    inputs = TC.waves4(mirrored, lossy)
    got = nat.sweep_host(inputs["dbeta"], extra_flags=LAYOUTS[layout], **sweep_kw(inputs))
    if mirrored:      # mirrored inputs give mirrored outputs bit for bit (in the mirrored loop and in the general one alike)
        assert np.array_equal(got["a_end"][:, 1], got["a_end"][:, 0]) and np.array_equal(got["a_end"][:, 3], got["a_end"][:, 2])
    frame = layout == "one_lane"
    meets_the_bar(check("waves4", f"{layout}-{'mirrored' if mirrored else 'general'}-{'lossy' if lossy else 'lossless'}", got, inputs,
                        known=SIGNAL_POWER if frame else (), budget=inputs["n_steps"] * R_OFF_UNIT if frame else 0.0))


@pytest.mark.parametrize("mirrored", [False, True])
def test_four_waves_one_lane_without_mismatch(mirrored):
    """The contrast that places the finding above: dbeta = 0 makes r = 1 exactly, and the same layout on the same fibre
    meets the bar.  (The two- and four-lane layouts and LDS staging, which carry the phase factor instead, meet it too.)"""
    inputs = TC.waves4_without_mismatch(mirrored)
    got = nat.sweep_host(inputs["dbeta"], extra_flags=nat.OPT_ONE_LANE, **sweep_kw(inputs))
    meets_the_bar(check("waves4", f"one_lane-{'mirrored' if mirrored else 'general'}-lossy-dbeta0", got, inputs))


G8_DRIFT = xfail(FRAME_DRIFT, "a_end max 1.7e-12 (8.7x the twin's), p_end median 3.3e-15 (16x..21x), p_max median 9.5e-16 (20x)")


@pytest.mark.parametrize("mirrored,alpha_i", [(False, 0), pytest.param(False, 1, marks=G8_DRIFT), (True, 0),
                                              pytest.param(True, 1, marks=G8_DRIFT)])
def test_four_waves_at_10000_steps_on_the_g8_inputs(mirrored, alpha_i):
    """10 000 steps of drift reach a_end as well (its maximum, at the points whose sidebands have grown to the pumps' scale):
    every output may miss by the stated drift and no more."""
    inputs = TC.g8(mirrored, alpha_i)
    got = nat.sweep_host(inputs["dbeta"], extra_flags=nat.OPT_ONE_LANE, **sweep_kw(inputs))
    if mirrored:      # the split of the figure the parity tests quote against the golden: whose error it is, element by element
        truth, golden = inputs["truth"]["a_end"], inputs["golden"]
        print(f"\ntruth | waves4-g8 | golden-split-a{alpha_i} | elementwise: kernel against the golden "
              f"{T.elementwise_err(got['a_end'], golden):.2e}, kernel against the yardstick {T.elementwise_err(got['a_end'], truth):.2e}"
              f", golden against the yardstick {T.elementwise_err(golden, truth):.2e}")
    meets_the_bar(check("waves4-g8", f"one_lane-{'mirrored' if mirrored else 'general'}-a{alpha_i}", got, inputs,
                        known=("a_end",) + SIGNAL_POWER, budget=inputs["n_steps"] * R_OFF_UNIT))


@pytest.mark.parametrize("layout", ["one_lane", "split"])
def test_six_waves(layout):
    inputs = TC.waves6()
    got = nat.sweep_host(inputs["dbeta"], dbeta2=inputs["dbeta2"], extra_flags=LAYOUTS[layout], **sweep_kw(inputs))
    meets_the_bar(check("waves6", layout, got, inputs))


def test_per_wave_summary():
    """psa_rk4_sweep_waves_f64 in the layout a driver's call gets: every wave's end and maximum power."""
    inputs = TC.waves4(False, True)
    got = nat.sweep_host(inputs["dbeta"], wave_summary=True, **sweep_kw(inputs))
    assert got["p_wave_end"].shape == (TC.N, 4)
    meets_the_bar(check("waves4", "per-wave-summary", got, inputs))


# ---- K pairs, single pump, comb --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 16])
def test_pairs(K):
    inputs = TC.pairs(K)
    meets_the_bar(check("pairs", f"K{K}", nat.sweep_pairs_host(inputs["dbeta"], **sweep_kw(inputs)), inputs))


def test_pairs_rows():
    """The multi-channel sweep's trajectory form: one span through psa_rk4_pairs_chain_f64."""
    inputs = TC.pairs(3)
    got = nat.pairs_chain_host(inputs["dbeta"][None], n_steps=[inputs["n_steps"]], seg_len=[inputs["z_max"]],
                               save_every=inputs["save_every"], gamma=inputs["gamma"][None], alpha=inputs["alpha"][None],
                               a0=inputs["a0"], want_traj=True)
    assert got["traj"].shape == inputs["truth"]["rows"].shape
    meets_the_bar(check("pairs", "K3-rows", got, inputs))


@pytest.mark.parametrize("lossy", [True, False])
def test_single_pump(lossy):
    inputs = TC.at_stride(TC.single_pump(lossy), TC.SAVE_EVERY)
    meets_the_bar(check("single_pump", "lossy" if lossy else "lossless", nat.single_pump_host(inputs["dbeta"], **sweep_kw(inputs)), inputs))


def test_single_pump_rows_at_every_step():
    inputs = TC.at_stride(TC.single_pump(True), 1)
    got = nat.single_pump_host(inputs["dbeta"], want_traj=True, **sweep_kw(inputs))
    assert got["traj"].shape == (TC.N, TC.N_STEPS + 1, 3)
    meets_the_bar(check("single_pump", "rows-save_every-1", got, inputs))


COMB = [(M, True) for M in range(3, 13)] + [(M, False) for M in (3, 7, 10, 12)]
COMB_LONG = [4, 7]                    # the same family at 100 000 steps (further down)


@functools.lru_cache(maxsize=None)
def _comb(M, lossy):
    """-> the outputs of the case that miss the bar (one launch and one record line per case, whichever test asks first).
    From M = 4 on a_end may miss, by the carried factor's stated budget and no more."""
    inputs = TC.comb(M, lossy)
    got = nat.comb_host(inputs["kappa"], **sweep_kw(inputs))
    return check("comb", f"M{M}-{'lossy' if lossy else 'lossless'}", got, inputs, known=("a_end",) if M >= 4 else (),
                 budget=CARRIED_BUDGET if M >= 4 else 0.0)


@pytest.mark.parametrize("M,lossy", COMB)
def test_comb(M, lossy):
    """Every instantiation: first_bad_step, the twin at RTOL_F64, the power summaries at the bar, and a_end at the bar (M = 3,
    whose pump line has kappa = 0) or within the bar plus the carried factor's stated drift (M >= 4; the bar itself for
    these is test_comb_family_meets_the_bar)."""
    missed = _comb(M, lossy)
    if M < 4:
        meets_the_bar(missed)


@xfail(CARRIED_U)
def test_comb_family_meets_the_bar():
    """The bar on a_end for every comb case with M >= 4, as one finding."""
    missed = {}
    for M, lossy in COMB:
        if M >= 4:
            missed.update({f"M{M}-{'lossy' if lossy else 'lossless'} {k}": v for k, v in _comb(M, lossy).items()})
    for M in COMB_LONG:
        missed.update({f"M{M}-lossy at 100 000 steps {k}": v for k, v in _comb_long(M).items()})
    meets_the_bar(missed)


def test_comb_without_dispersion():
    """The contrast that places the finding above: kappa = 0 leaves u_m = 1 and every rotator (1, 0), nothing carried can
    drift, and M = 7 -- over the floor with dispersion -- sits with the twin."""
    inputs = TC.comb_without_dispersion(7)
    meets_the_bar(check("comb", "M7-lossy-kappa0", nat.comb_host(inputs["kappa"], **sweep_kw(inputs)), inputs))


# ---- 100 000 steps, float64: the step count the headline runs --------------------------------------------------------------
# 64 points (one wave of every lane layout; K = 16: 32 points, eight waves of its 16-lane groups) over 1000 m, the compiled
# 80-bit run as the yardstick and its double instantiation as the twin (oracle/plain_rk4.py, pinned in
# tests/test_truth_long_host.py).  The step count is what is under test: what a kernel carries between seeds must not accumulate.
EVERY_OUTPUT = ("a_end",) + SIGNAL_POWER
REGROUPING = 1e-13        # psa_rk4_kernel.inc.h: "the regrouping costs ~1 ulp(y) of rounding noise per step, ~1e-13 after 1e5 steps"
G8_LONG_A0 = xfail(FRAME_DRIFT, "at 1e5 steps a_end max 1.50e-11 (25x the twin's), p_end median 2.9e-14 (32x) max 1.1e-12 (9.7x), "
                                "p_max median 1.9e-14 (98x)")
G8_LONG_A1 = xfail(FRAME_DRIFT, "at 1e5 steps a_end max 1.40e-11 (19x the twin's; median 4.5x..4.8x), p_end median 2.9e-14 (49x) max 1.5e-12 (11x), "
                                "p_max median 5.7e-15..6.9e-15 (27x..33x); a_end's median by the fused step's regrouping, inside the "
                                "header's 1e-13 for it")
G8_LONG = [pytest.param("one_lane", False, 0, 10, marks=G8_LONG_A0), pytest.param("one_lane", False, 1, 10, marks=G8_LONG_A1),
           pytest.param("one_lane", True, 0, 10, marks=G8_LONG_A0), pytest.param("one_lane", True, 1, 10, marks=G8_LONG_A1),
           pytest.param("one_lane", True, 1, 7, marks=G8_LONG_A1),
           ("split", False, 0, 10), ("split", False, 1, 10), ("quad", False, 0, 10), ("quad", False, 1, 10),
           ("lds", False, 0, 10), ("lds", False, 1, 10)]


@pytest.mark.parametrize("layout,mirrored,alpha_i,save_every", G8_LONG)
def test_four_waves_at_100000_steps_on_the_g8_inputs(layout, mirrored, alpha_i, save_every):
    """save_every = 10 in the one-lane layout is the straight-line ten-step-row loop the benchmark runs, 7 the run-time row loop.
    The layouts that carry the phase factor between 64-step seeds meet the bar as they do at 1 500 steps: nothing accumulates
    across seeds.  The one-lane cases miss by the frame's drift, and the band on them is that drift EVALUATED: the kernel header's
    own |r| - 1 <= 5.5e-17 per step, planted into the 80-bit run of the same inputs (truth_cases.g8_long_frame_drift).  The plain
    product n (|r| - 1) = 5.5e-12, which the header used to quote as the effect after 1e5 steps, holds for the sidebands' moduli
    while the pumps are undepleted; on the points of this set where the sidebands have reached a tenth of the pumps the
    propagation carries the same drift to 1.5e-11 of the largest wave (the kernel: 1.50e-11 / 1.40e-11 at alpha = 0 / > 0; each
    lane's own |r| planted on the CPU: 1.46e-11 / 1.33e-11; the bound 5.5e-17 in every lane, the band: 2.07e-11 / 1.75e-11).
    The band on a MEDIAN is the planted run's median (4.7e-14..6.0e-14 on a_end), not its maximum.  That drift does not carry
    a_end's median at alpha > 0 (6.6e-13, 4.5x..4.8x the twin's 1.4e-13): half the points have no sidebands to speak of.  What
    does is the fused step's regrouping, for which the same header states ~1e-13 after 1e5 steps; a_end's band has both."""
    inputs = TC.g8_long(mirrored, alpha_i, save_every)
    got = nat.sweep_host(inputs["dbeta"], extra_flags=LAYOUTS[layout], **sweep_kw(inputs))
    if mirrored:
        assert np.array_equal(got["a_end"][:, 1], got["a_end"][:, 0]) and np.array_equal(got["a_end"][:, 3], got["a_end"][:, 2])
    frame = layout == "one_lane"
    case = f"{layout}-{'mirrored' if mirrored else 'general'}-a{alpha_i}" + ("" if save_every == 10 else f"-save_every-{save_every}")
    budget = TC.g8_long_frame_drift(mirrored, alpha_i, save_every, R_OFF_UNIT) if frame else 0.0
    if frame:
        print(f"\ntruth | waves4-g8-1e5 | {case} | the stated |r| - 1 = {R_OFF_UNIT:.1e} per step planted into the 80-bit run: "
              + ", ".join(f"{k} median {v[0]:.2e} max {v[1]:.2e}" for k, v in budget.items())
              + f" (n (|r| - 1) = {inputs['n_steps'] * R_OFF_UNIT:.1e}); a_end's band adds the regrouping's {REGROUPING:.0e}", end="")
        budget = dict(budget, a_end=tuple(b + REGROUPING for b in budget["a_end"]))
    meets_the_bar(check("waves4-g8-1e5", case, got, inputs, known=EVERY_OUTPUT if frame else (), budget=budget))


@pytest.mark.parametrize("layout", ["one_lane", "split"])
def test_six_waves_at_100000_steps(layout):
    inputs = TC.waves6_long()
    got = nat.sweep_host(inputs["dbeta"], dbeta2=inputs["dbeta2"], extra_flags=LAYOUTS[layout], **sweep_kw(inputs))
    meets_the_bar(check("waves6-1e5", layout, got, inputs))


@pytest.mark.parametrize("K", [3, 16])
def test_pairs_at_100000_steps(K):
    """K = 3: a padded group of four lanes; K = 16: the widest group."""
    inputs = TC.pairs_long(K)
    meets_the_bar(check("pairs-1e5", f"K{K}", nat.sweep_pairs_host(inputs["dbeta"], **sweep_kw(inputs)), inputs))


def test_single_pump_at_100000_steps():
    inputs = TC.single_pump_long()
    meets_the_bar(check("single_pump-1e5", "lossy", nat.single_pump_host(inputs["dbeta"], **sweep_kw(inputs)), inputs))


@functools.lru_cache(maxsize=None)
def _comb_long(M):
    inputs = TC.comb_long(M)
    return check("comb-1e5", f"M{M}-lossy", nat.comb_host(inputs["kappa"], **sweep_kw(inputs)), inputs)


@pytest.mark.parametrize("M", COMB_LONG)
def test_comb_at_100000_steps(M):
    """Every output at the bar, a_end included: the carried factor's drift between two seeds (1.4e-14) does not grow with the
    number of seeds and is far inside a plain RK4's own 1e-13 here, so these cases need no band (M4 2.1x / 0.9x, M7 1.8x / 2.0x
    of the twin).  They are still listed in the family's test, where they add nothing to what it expects."""
    meets_the_bar(_comb_long(M))


def test_comb_without_dispersion_at_100000_steps():
    inputs = TC.comb_long(7, False)
    meets_the_bar(check("comb-1e5", "M7-lossy-kappa0", nat.comb_host(inputs["kappa"], **sweep_kw(inputs)), inputs))


# ---- chains ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["waves", "single_pump", "pairs", "comb"])
def test_chain(family):
    inputs = TC.chain(family)
    kw = TC.chain_arrays(inputs)
    dbeta = kw.pop("dbeta")
    if family == "waves":
        got = nat.chain_host(dbeta, want_traj=True, **kw)
    elif family == "single_pump":
        got = nat.single_pump_chain_host(dbeta, want_traj=True, **kw)
    elif family == "comb":
        got = nat.comb_chain_host(dbeta, want_traj=True, **kw)
    else:
        got = nat.pairs_chain_host(dbeta, want_traj=True, **kw)
    assert got["traj"].shape == inputs["truth"]["rows"].shape
    meets_the_bar(check("chain", family, got, inputs))


# Three spans of the 4/6-wave chain entry point (truth_cases.chain3*): both pairs' gauge (theta2 / dbeta2 of the epilogue) under
# transfers on every wave, the forced lane layouts, the per-wave summary, and a middle span that ends before the first re-seed.
# Two launches per case: the trajectory (a_end, p_end, p_max, rows) and the per-wave summary (a_end, p_wave_end, p_wave_max).
def _chain3_launches(inputs, flags, dtype=np.float64):
    kw = TC.chain_arrays(inputs)
    dbeta = kw.pop("dbeta")                                     # (S, N, K): column 0 the first pair's, column 1 the second's
    kw.update(dtype=dtype, extra_flags=flags, dbeta2=np.ascontiguousarray(dbeta[:, :, 1]) if dbeta.shape[2] == 2 else None)
    dbeta = np.ascontiguousarray(dbeta[:, :, 0])
    rows, waves = nat.chain_host(dbeta, want_traj=True, **kw), nat.chain_host(dbeta, wave_summary=True, **kw)
    assert rows["traj"].shape == inputs["truth"]["rows"].shape and waves["p_wave_end"].shape == inputs["a0"].shape
    return {k: rows[k] for k in ("a_end", "p_end", "p_max", "traj", "first_bad_step")}, \
           {k: waves[k] for k in ("a_end", "p_wave_end", "p_wave_max", "first_bad_step")}


def _pump_powers_meet_the_bar(got, inputs, floor):
    """The per-wave powers of the two pumps alone (truth_cases.pump_power_errors): under the bar itself."""
    e_got, e_twin = TC.pump_power_errors(got, inputs["truth"]), TC.pump_power_errors(inputs["twin"], inputs["truth"])
    for key in e_got:
        assert TC.bar(e_got[key], e_twin[key], floor)[0], f"{key} of the pumps misses the bar"


CHAIN3_F64 = [(4, False, "one_lane"), (4, False, "split"), (4, False, "quad"), (4, True, "one_lane"), (6, False, "one_lane"),
              (6, False, "split")]


@pytest.mark.parametrize("n_waves,mirrored,layout", CHAIN3_F64)
def test_chain_of_three_spans(n_waves, mirrored, layout):
    """Float64, 460 + 40 + 1000 steps.  Mirrored: span 0 runs the mirrored loop, spans 1 and 2 the general one.

    The one-lane four-wave step is frame-anchored (FRAME_DRIFT above), in a chain as in a sweep: in those two cases the signal's
    power -- p_end / p_max, and the per-wave powers where waves 2 and 3 carry them past the bar -- is held to the band
    test_four_waves holds it to, the bar plus 1 500 (|r| - 1) by the header's figure; a_end, the rows and the pumps' powers are
    held to the bar itself, and nothing lies beyond the band.  (Measured: neither case needs the band.  p_end is 15x and
    8.5x the twin's median and, at 4e-16, under the floor.)"""
    inputs = TC.chain3(n_waves, mirrored)
    rows, waves = _chain3_launches(inputs, LAYOUTS[layout])
    case = f"{TC.chain3_name(n_waves, mirrored)}-{layout}"
    frame = layout == "one_lane" and n_waves == 4
    budget = sum(s[1] for s in inputs["spans"]) * R_OFF_UNIT if frame else 0.0
    missed = check("chain3", case + "-rows", rows, inputs, known=SIGNAL_POWER if frame else (), budget=budget)
    missed_w = check("chain3", case + "-per-wave", waves, inputs, known=("p_wave_end", "p_wave_max") if frame else (), budget=budget)
    if missed_w:
        _pump_powers_meet_the_bar(waves, inputs, TC.FLOOR_F64)
        print(f"truth | chain3 | {case}-per-wave | {', '.join(missed_w)} between the bar and the band by waves 2 and 3 (the frame's drift, "
              f"budget {budget:.2e}); the pumps' own meet the bar")
    if not frame:
        meets_the_bar(dict(missed, **missed_w))


# ---- float32 ---------------------------------------------------------------------------------------------------------------
# Two bars.  The first, as above: no worse than a PLAIN float32 RK4 (floor 2e-6), with RTOL_F32 against the yardstick beside it.
# The kernels sit 12x..30x below that twin, so it cannot see a compensated state that got lost.  The second holds the kernel to
# the compensated float32 statement of its own kind -- Kahan for the scalar kernel, base + offset with a fold every 16 steps for
# the packed ones (oracle/psa_plain_rk4.c) -- with NO floor, by the factors 4 and 8 on a_end and on every wave's power and by
# 9.71 and 8 on wave 2's power alone, three times what the two compensated statements themselves differ by there
# (truth_cases.bar_compensated; factors and planted defects: tests/test_truth_long_host.py).  The yardstick of the long cases is the compiled double run of the rounded inputs.
F32_LAYOUTS = dict(packed=(nat.OPT_F32_PACKED, "base_offset"), scalar=(nat.OPT_F32_SCALAR, "kahan"))


def check_float32(family, case, got, inputs, kind, plain_launch=None, known=(), budget=None):
    """Both float32 bars, every assertion of check included; the second on a_end and on every wave's end and maximum power.
    ``plain_launch``: the same sweep without the per-wave summary (the instantiation the benchmark runs): its a_end and wave
    2's p_end / p_max are held to the second bar too, the latter two by the factors of one wave alone
    (truth_cases.factors_compensated).  A ``plain_launch`` with a trajectory (a chain's) goes through check as well, and its
    rows are judged under both bars.  Raises BarMissed for what misses either bar.

    ``known`` (with ``budget``, {output: (median, maximum)}): the outputs of the PLAIN launch a documented design choice lets miss
    the SECOND bar.  Then BarMissed can carry these outputs and nothing else: everything else -- the first bar of both launches,
    the second bar of the whole per-wave launch and of the plain launch's other outputs, and the band on the known ones, that bar
    plus the budget (from the kernel header's figure, never a kernel's) -- fails with a plain AssertionError, which a strict xfail
    on BarMissed does not accept.  Without ``known`` nothing changes: every miss of either bar is a BarMissed."""
    assert got["a_end"].dtype == np.complex64 and got["p_wave_end"] is not None
    missed = check(family, case, got, inputs, TC.FLOOR_F32, RTOL_F32)
    second = TC.judge_compensated(family, case, got, inputs, kind)
    if plain_launch is not None:
        assert (plain_launch["first_bad_step"] == -1).all()
        keys = ("a_end", "p_end", "p_max")
        if plain_launch.get("traj") is not None:
            keys += ("traj",)
            missed.update({f"{k} of the trajectory launch": v for k, v in
                           check(family, case + "-plain-launch", plain_launch, inputs, TC.FLOOR_F32, RTOL_F32).items()})
        second_plain = TC.judge_compensated(family, case + "-plain-launch", {k: plain_launch[k] for k in keys}, inputs, kind)
        if known:
            assert not missed, "the first bar: " + "\n".join(line for line, *_ in missed.values())
            assert not second, "the second bar, per-wave launch: " + "\n".join(line for line, *_ in second.values())
            assert set(second_plain) <= set(known), "\n".join(second_plain[k][0] for k in second_plain if k not in known)
            for key, (line, med, mx, tmed, tmx) in second_plain.items():
                f_med, f_max = TC.factors_compensated(key)
                assert med <= f_med * tmed + budget[key][0] and mx <= f_max * tmx + budget[key][1], f"beyond the stated drift: {line}"
        second.update({f"{k} without the per-wave summary": v for k, v in second_plain.items()})
    else:
        assert not known
    meets_the_bar(missed)
    meets_the_bar({f"{k} against the {kind} twin": v for k, v in second.items()})


@pytest.mark.parametrize("layout,mirrored", [("packed", False), ("packed", True), ("scalar", False)])
def test_four_waves_float32(layout, mirrored):
    inputs = TC.waves4_f32(mirrored)
    got = nat.sweep_host(inputs["dbeta"], dtype=np.float32, extra_flags=F32_LAYOUTS[layout][0], **sweep_kw(inputs))
    assert got["a_end"].dtype == np.complex64
    meets_the_bar(check("waves4-f32", f"{layout}-{'mirrored' if mirrored else 'general'}", got, inputs, TC.FLOOR_F32, RTOL_F32))


def test_single_pump_float32():
    inputs = TC.single_pump_f32()
    got = nat.single_pump_host(inputs["dbeta"], dtype=np.float32, **sweep_kw(inputs))
    assert got["a_end"].dtype == np.complex64
    meets_the_bar(check("single_pump-f32", "packed", got, inputs, TC.FLOOR_F32, RTOL_F32))


def _sweep_f32(inputs, flags, wave_summary):
    return nat.sweep_host(inputs["dbeta"], dbeta2=inputs.get("dbeta2"), dtype=np.float32, extra_flags=flags, wave_summary=wave_summary,
                          **sweep_kw(inputs))


@pytest.mark.parametrize("layout,mirrored", [("packed", False), ("packed", True), ("scalar", False)])
def test_four_waves_float32_against_the_compensated_twin(layout, mirrored):
    """The 1 500-step sets above under both bars, in a launch with the per-wave summary and in one without.  On the general set
    the kernels' p_max sits at 4.0x..4.6x of the twin's median, inside the 9.71 that the two compensated statements' own spread
    on one wave's power sets: the float32 kernels carry the phase factor between 16-step seeds where the twins take cosf / sinf
    at every stage."""
    inputs = TC.waves4_f32_compensated(mirrored)
    flags, kind = F32_LAYOUTS[layout]
    check_float32("waves4-f32", f"{layout}-{'mirrored' if mirrored else 'general'}", _sweep_f32(inputs, flags, True), inputs, kind,
                  plain_launch=_sweep_f32(inputs, flags, False))


def test_single_pump_float32_against_the_compensated_twin():
    inputs = TC.single_pump_f32_compensated()
    got = nat.single_pump_host(inputs["dbeta"], dtype=np.float32, **sweep_kw(inputs))
    check_float32("single_pump-f32", "packed", got, inputs, "base_offset")


CARRIED_BUDGET_F32 = 2 * TC.F32_RESYNC * 2.0 ** -24    # psa_rk4_kernel.inc.h's rule for a carried factor, "drift <= 128
#   multiplications ~1.4e-14" between two float64 seeds 64 steps apart (2 x 64 roundings of 2^-53), at the float32 kernels' 16
#   steps and 2^-24: 1.9e-6
CARRIED_E_F32 = (
    "the float32 kernels carry E(z) = 2 gamma exp(i dbeta z) by one rounded rotation per half step between exact seeds 16 steps "
    "apart (psa_rk4_kernel.inc.h) where the compensated twins take cosf / sinf at every stage (DESIGN.md 4): up to 32 roundings "
    "in E, 1.9e-6 by that header's rule for a carried factor (stated there for float64; the float32 figure is the same rule at 16 "
    "steps and 2^-24), which a span with parametric gain carries into the signal.  On the four-wave general chain ONE point, "
    "nearly phase-matched over its last span with the signal grown towards the pumps, decides the maxima of wave 2's power alone "
    "(each run's record line names it).  The same carried factor planted into the Kahan chain twin on the CPU takes its p_end / "
    "p_max maxima from 2.9e-8 / 2.5e-8 to 2.5e-7 / 2.2e-7, the kernels' figures, at that point, and moves nothing else "
    "(test_truth_long_host.test_a_carried_phase_factor_takes_the_signal_power_over_the_second_bar): the compensated state and "
    "the chain's boundaries are not involved.  This mark stands in for a fix that has not been made.  "
    "Measured: ")
CHAIN3_F32 = [
    pytest.param(4, False, "packed", marks=xfail(CARRIED_E_F32, "p_max max 2.57e-7 (10.8x the base + offset twin's; p_end 2.99e-7, 6.9x)")),
    pytest.param(4, False, "scalar", marks=xfail(CARRIED_E_F32, "p_end max 2.65e-7 (9.2x the Kahan twin's), p_max max 2.28e-7 (9.2x)")),
    (4, True, "packed"), (6, False, "packed"), (6, False, "scalar")]


@pytest.mark.parametrize("n_waves,mirrored,layout", CHAIN3_F32)
def test_chain_of_three_spans_float32(n_waves, mirrored, layout):
    """Float32, 460 + 12 + 1028 steps, rows every 4, both bars on both launches.  The middle span ends before the first 16-step
    seed and fold: what the boundary carries is a base with an unfolded offset, rotated and rounded, transferred and rounded.
    A chain whose spans >= 1 had lost the compensated state would sit at 2.5x .. 4.4x the second bar
    (test_truth_long_host.test_the_second_bar_sees_a_compensation_lost_at_a_boundary).

    On the four-wave general set wave 2's power alone (p_end / p_max of the trajectory launch) may miss the second bar by what
    the carried phase factor's drift does to it, and no more; that band is the drift EVALUATED: E off by 2 x 16 x 2^-24 in
    modulus at every z, planted into the 80-bit chain of the same inputs (truth_cases.chain3_f32_coupling_drift).  The band is
    LOOSE and says so: the kernel header states the carried factor's figure for float64 only, 1.9e-6 is its rule at float32's 16
    steps and 2^-24, and a drift of that size with one sign at every z gives 1.6e-6 / 1.4e-6 on the maxima -- six times what the
    kernels show and about the first bar's floor -- so on these two outputs of these two cases the band catches a gross change
    and little else.  What the mark cannot hide is everything else: BarMissed can carry p_end / p_max of the trajectory launch
    alone (check_float32); every other output of both launches under both bars, the yardstick at RTOL_F32 and first_bad_step
    fail the case with a plain AssertionError."""
    inputs = TC.chain3_f32(n_waves, mirrored)
    flags, kind = F32_LAYOUTS[layout]
    rows, waves = _chain3_launches(inputs, flags, np.float32)
    assert rows["traj"].dtype == np.complex64
    case = f"{TC.chain3_name(n_waves, mirrored)}-{layout}"
    carried = n_waves == 4 and not mirrored
    budget = TC.chain3_f32_coupling_drift(n_waves, mirrored, CARRIED_BUDGET_F32) if carried else None
    if carried:
        print(f"\ntruth | chain3-f32 | {case} | E off by the stated {CARRIED_BUDGET_F32:.1e} planted into the 80-bit chain: "
              + ", ".join(f"{k} median {budget[k][0]:.2e} max {budget[k][1]:.2e}" for k in SIGNAL_POWER), end="")
        print(f"\ntruth | chain3-f32 | {case} | " + TC.chain3_signal_report(rows["p_end"], rows["p_max"], rows["traj"], inputs), end="")
    check_float32("chain3-f32", case, waves, inputs, kind, plain_launch=rows, known=SIGNAL_POWER if carried else (), budget=budget)


CONFIG4 = [("mirrored", 100_000, "packed"), ("mirrored", 1_000_000, "packed"), ("general", 100_000, "packed"),
           ("general", 1_000_000, "packed"), ("general", 100_000, "scalar"), ("strong", 100_000, "packed"), ("six", 100_000, "packed")]


@pytest.mark.parametrize("powers,n_steps,layout", CONFIG4)
def test_float32_config4_shaped(powers, n_steps, layout):
    """17 points (8 packed lanes and the odd tail), dbeta from -0.02 to 0.02 over 1000 m, rows every 10 steps: config 4's powers
    (the mirrored loop) at its 1e6 steps and at 1e5, the general loop on (0.1, 0.08, 1e-7, 1e-7), the scalar kernel, 0.5 / 0.4 W
    pumps with 1e-5 W sidebands, and six waves.  Two launches: with the per-wave summary, and the benchmark's own without."""
    inputs = TC.config4_f32(powers, n_steps)
    flags, kind = F32_LAYOUTS[layout]
    got, plain = _sweep_f32(inputs, flags, True), _sweep_f32(inputs, flags, False)
    if powers == "mirrored":
        for g in (got, plain):
            assert np.array_equal(g["a_end"][:, 1], g["a_end"][:, 0]) and np.array_equal(g["a_end"][:, 3], g["a_end"][:, 2])
    check_float32("config4-f32", f"{layout}-{powers}-{n_steps}", got, inputs, kind, plain_launch=plain)


@pytest.mark.parametrize("n_steps", [100_000, 1_000_000])
def test_single_pump_float32_long(n_steps):
    inputs = TC.single_pump_f32_long(n_steps)
    got = nat.single_pump_host(inputs["dbeta"], dtype=np.float32, **sweep_kw(inputs))
    check_float32("single_pump-f32", f"packed-{n_steps}", got, inputs, "base_offset")
