"""The compiled plain RK4 (oracle/psa_plain_rk4.c through oracle/plain_rk4.py) without a GPU, before anything leans on it: its
80-bit instantiation is the yardstick of the 1e5-step cases of tests/test_gpu_truth.py, its double one their twin and the
yardstick of the float32 cases, its float ones -- plain, Kahan, base + offset -- the float32 twins.

Pinned here: the 80-bit instantiation against truth_ld (another operation order in the same arithmetic) and against 40-digit
mpmath; the double and the plain float instantiation against the twins tests/test_truth_host.py already holds; how far the two
compensated float32 statements lie apart, which sets the factors of the second float32 bar; that the bar, as the GPU cases
apply it, fails a float32 run that dropped its compensation or throws the fold's residue away, at every step count it is
applied at; the same for the float32 three-span chains (truth_cases.chain3_f32), whose planted defect is a compensation lost at
a span boundary, and the plant that places their one finding, the carried phase factor; and the conditioning of every 1e5-step
input set.  Every test prints its figures (record: profiles/truth_errors.txt)."""
import mpmath
import numpy as np
import pytest

import plain_rk4
import test_truth_host as H
import truth_cases as TC
import truth_ld as T

EPS_LD = 1.1e-19                       # 2^-63: the spacing of x87 extended at 1
SPREAD_MED, SPREAD_MAX = 1.3, 2.4      # two plain statements of one scheme in one precision (tests/test_truth_host.py)


def _c(model, s, rate, precision, update="plain", **over):
    kw = dict(z_max=s["z_max"], n=s["n_steps"], save_every=s.get("save_every", 1), gamma=s["gamma"], alpha=s["alpha"])
    kw.update(over)
    return plain_rk4.integrate(model, s["a0"], rate, precision=precision, update=update, **kw)


def _rate(s):
    return s["kappa"] if "kappa" in s else TC._rate2(s)


# (name, model, set): the 1 500-step sets of every model the C text covers; one K per lane-group width (2, 4, 8, 16)
SETS_1500 = ([("waves4-general-lossy", "pairs", lambda: TC.waves4(False, True)), ("waves4-mirrored-lossless", "pairs", lambda: TC.waves4(True, False)),
              ("waves6", "pairs", TC.waves6)]
             + [(f"pairs-K{K}", "pairs", lambda K=K: TC.pairs(K)) for K in (2, 3, 8, 16)]
             + [("single_pump-lossy", "single_pump", lambda: TC.single_pump(True))]
             + [(f"comb-M{M}-lossy", "comb", lambda M=M: TC.comb(M, True)) for M in (3, 7, 12)])


# ---- the 80-bit instantiation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,inputs", SETS_1500, ids=[n for n, _, _ in SETS_1500])
def test_c_yardstick_against_truth_ld(name, model, inputs):
    """Two 80-bit runs of one scheme in different operation orders (truth_ld states the pair model in the pairs kernel's form and
    sums the comb's products through NumPy; the C text states yaman_model's form and loops).  How far apart they can lie, worked
    out and not measured: a step rounds the updated state once (half a spacing, 0.5 eps of the wave) and adds an increment that
    is itself h |f| <= 1e-2 of the state with some tens of roundings behind it (under 0.5 eps of the state): at most 1 eps per
    step and run, 2 eps for the distance of two runs, n of them in line if every one had the same sign, and a factor 2 for what
    the propagation makes of an earlier error (the sets are conditioned: TWIN_CONDITION) -- 4 n eps, 6.6e-16 at 1 500 steps,
    still 20 times finer than a float64 twin resolves.  Roundings random-walk, so the measured distance is far below."""
    s = inputs()
    got = _c(model, s, _rate(s), "ld", want_rows=s["truth"]["rows"] is not None)
    assert got["a_end"].dtype == np.clongdouble and got["p_wave_max"].dtype == np.longdouble
    e = TC.errors(got, s["truth"])
    bound = 4 * s["n_steps"] * EPS_LD
    print(f"\nc-ld | {name} | bound {bound:.2e} | " + " | ".join(f"{k} median {np.median(v):.2e} max {v.max():.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v.max() <= bound, k


MP_MODEL = {"waves4": "pairs", "pairs-K3": "pairs", "single_pump": "single_pump", "comb-M4": "comb"}


@pytest.mark.parametrize("name", list(H.MP_CASES))
def test_c_yardstick_against_40_digit_arithmetic(name):
    """The short runs of test_truth_host's mpmath check (point 0 of the model's set, 8 steps of 3.75 m), held to the same 1e-17."""
    f_mp, _, inputs, rate_key = H.MP_CASES[name]
    inp = inputs()
    rate = np.atleast_1d(inp[rate_key][0])
    a0, gamma, alpha = inp["a0"][0], inp["gamma"][0], inp["alpha"][0]
    with mpmath.workdps(40):
        want = H._mp_rk4(f_mp, a0, rate, gamma, alpha, 30.0, 8)
        got = plain_rk4.integrate(MP_MODEL[name], a0[None, :], rate[None, :], z_max=30.0, n=8, save_every=8, gamma=gamma, alpha=alpha,
                                  precision="ld")["a_end"][0]
        err = max(abs(mpmath.mpc(H._to_mp(x.real), H._to_mp(x.imag)) - w) for x, w in zip(got, want)) / max(abs(w) for w in want)
    print(f"\nc-ld | {name}: C 80-bit run against 40 digits {float(err):.2e} of the largest wave")
    assert err < 1e-17


def test_rows_follow_integrate_fixed_step():
    """Row 0 at z = 0, a row after every step with (i + 1) % save_every == 0, a_end the last saved row -- with a tail behind it."""
    s = TC.waves4(False, True)
    every = _c("pairs", s, s["dbeta"], "f64", n=30, z_max=6.0, save_every=1, want_rows=True)
    some = _c("pairs", s, s["dbeta"], "f64", n=30, z_max=6.0, save_every=7, want_rows=True)
    assert some["rows"].shape == (TC.N, 5, 4)
    assert np.array_equal(some["rows"], every["rows"][:, ::7]) and np.array_equal(some["a_end"], every["rows"][:, 28])
    assert np.array_equal(some["rows"][:, 0], np.asarray(s["a0"]))
    p = np.abs(every["rows"][:, ::7]) ** 2
    assert np.allclose(some["p_wave_max"], p.max(axis=1), rtol=1e-15) and np.allclose(some["p_wave_end"], p[:, -1], rtol=1e-15)


def test_planted_sideband_drift_is_n_times_the_step_factor_while_the_pumps_are_undepleted():
    """The facility the one-lane band is evaluated with (truth_cases.g8_long_frame_drift): sidebands scaled by 1 + d after every
    step.  G8's inputs over 100 m, where the sidebands' power stays below 1e-4 of the pumps' and the equations are linear in
    them to that order: their moduli end n d off, the pumps unmoved, both to O(P_s / P_p) of n d (bounds: 1e-3)."""
    s, n, d = TC.g8_inputs(1), 2000, 1e-12
    kw = dict(z_max=100.0, n=n, save_every=n, gamma=s["gamma"], alpha=s["alpha"], precision="ld")
    clean = plain_rk4.integrate("pairs", s["a0"], s["dbeta"], **kw)["a_end"]
    planted = plain_rk4.integrate("pairs", s["a0"], s["dbeta"], sideband_drift=d, **kw)["a_end"]
    ratio = np.abs(planted) / np.abs(clean) - 1
    print(f"\ndrift | sidebands {float(ratio[:, 2:].min()):.6e} .. {float(ratio[:, 2:].max()):.6e} (n d = {n * d:.1e}), pumps up to "
          f"{float(np.abs(ratio[:, :2]).max()):.1e}")
    assert np.allclose(np.asarray(ratio[:, 2:], dtype=float), n * d, rtol=1e-3) and np.abs(ratio[:, :2]).max() < 1e-3 * n * d
    with pytest.raises(ValueError):
        plain_rk4.integrate("pairs", s["a0"], s["dbeta"], sideband_drift=d, **dict(kw, precision="f32"), update="kahan")


# ---- the double and the plain float instantiation: plain statements among the plain statements -------------------------------
def _within_the_spread(tag, name, e_c, e_twin):
    """a_end's errors against the yardstick (the output test_truth_host's spread is recorded on), both ways."""
    print(f"\n{tag} | {name} | " + " | ".join(f"{k} C {np.median(e_c[k]):.2e} {e_c[k].max():.2e} twin {np.median(e_twin[k]):.2e} "
                                              f"{e_twin[k].max():.2e}" for k in e_c))
    med, mx = np.median(e_c["a_end"]) / np.median(e_twin["a_end"]), e_c["a_end"].max() / e_twin["a_end"].max()
    assert max(med, 1 / med) <= SPREAD_MED and max(mx, 1 / mx) <= SPREAD_MAX, (med, mx)


F64_1500 = [(n, f) for n, f in TC.F64_SETS if not n.startswith("chain")]


@pytest.mark.parametrize("name,inputs", F64_1500, ids=[n for n, _ in F64_1500])
def test_c_double_twin_is_a_plain_statement(name, inputs):
    """Every float64 input set of one span: the C double run's errors against the yardstick lie within the spread of two plain
    float64 statements (medians 1.3x, maxima 2.4x) of the set's own twin's.

    Measured: all 36 sets within 1.21x on the median and 1.19x on the maximum.  That took a correction of the text: with ONE
    rounded h = z_max / n for every step, 35 sets were inside and pairs-K8 sat at 1.44x on the median (5.68e-15 against
    pairs_np's 3.94e-15), and no reordering of the right-hand side or of the k1..k4 combination moved it (1.41x..1.46x: the
    increment is 1e-2 of the state, its last bits rarely change fl(y + increment)).  The twins, like integrate_fixed_step, take
    the step as the difference of its two grid points (np.linspace, h = z[i + 1] - z[i]); so does the text now, and its double
    instantiation follows the NumPy twins' rounding path (pairs, single pump, comb: 0.90x..1.14x)."""
    s = inputs()
    model = "comb" if "kappa" in s else "single_pump" if s["a0"].shape[-1] == 3 else "pairs"
    got = _c(model, s, _rate(s), "f64", want_rows=s["truth"]["rows"] is not None)
    _within_the_spread("c-f64", name, TC.errors(got, s["truth"]), TC.errors(s["twin"], s["truth"]))


@pytest.mark.parametrize("name,inputs", TC.F32_SETS, ids=[n for n, _ in TC.F32_SETS])
def test_c_plain_float_is_rk4_f32(name, inputs):
    s = inputs()
    got = _c("single_pump" if s["a0"].shape[-1] == 3 else "pairs", s, s["dbeta"], "f32")
    assert got["a_end"].dtype == np.complex64 and got["p_wave_end"].dtype == np.float32
    _within_the_spread("c-f32", name, TC.errors(got, s["truth"]), TC.errors(s["twin"], s["truth"]))


# ---- float32: the compensated statements and the second bar ------------------------------------------------------------------
def _single_wave_form(res):
    """Wave 2's p_end / p_max alone, what sweep_host returns without the per-wave summary."""
    return dict(a_end=res["a_end"], p_end=res["p_wave_end"][:, 2], p_max=res["p_wave_max"][:, 2])


def _every_output(res, truth):
    """Errors of everything a GPU case holds to the second bar: a_end and every wave's power (the launch with the per-wave
    summary), and wave 2's p_end / p_max alone (the launch without it; not for the single-pump model, which has no such launch)."""
    e = TC.errors(res, truth)
    if res["a_end"].shape[-1] != 3:
        e.update({k: v for k, v in TC.errors(_single_wave_form(res), truth).items() if k != "a_end"})
    return e


@pytest.mark.parametrize("name,inputs", TC.F32_COMPENSATED_SETS, ids=[n for n, _ in TC.F32_COMPENSATED_SETS])
def test_spread_of_the_compensated_statements(name, inputs):
    """Kahan and base + offset against the yardstick, on every output the second bar is applied to: their medians and maxima lie
    within a third of that output's factors of each other -- which is what sets the factors, as in float64.  Measured: a_end and
    every wave's power within 1.28x (medians) and 1.56x (maxima): factors 4 and 8.  Wave 2's power alone: maxima within 1.22x,
    factor 8; medians up to 3.2345x apart (0.5 / 0.4 W pumps, 1e5 steps), beyond 4 / 3, so that factor is three times the
    measured spread, 9.71 (truth_cases.F32C_ONE_WAVE_MED)."""
    s = inputs()
    e_k, e_b = _every_output(s["kahan"], s["truth"]), _every_output(s["base_offset"], s["truth"])
    ratio = {k: (max(np.median(e_k[k]) / np.median(e_b[k]), np.median(e_b[k]) / np.median(e_k[k])),
                 max(e_k[k].max() / e_b[k].max(), e_b[k].max() / e_k[k].max())) for k in e_k}
    print(f"\nspread-f32 | {name} | " + " | ".join(
        f"{k} kahan {np.median(e_k[k]):.2e} {e_k[k].max():.2e} base+offset {np.median(e_b[k]):.2e} {e_b[k].max():.2e} ratio "
        f"{ratio[k][0]:.4f} {ratio[k][1]:.4f}" for k in e_k))
    for k, (r_med, r_max) in ratio.items():
        f_med, f_max = TC.factors_compensated(k)
        assert r_med <= f_med / 3 and r_max <= f_max / 3, k


def _margin(planted, twin_c, truth):
    """How far a planted run misses the second bar, as the GPU case would judge it: the largest of ratio / factor over its
    outputs' medians and maxima (> 1: it misses)."""
    e_p, e_t = _every_output(planted, truth), _every_output(twin_c, truth)
    worst, missed = 0.0, False
    for k in e_p:
        ok, r_med, r_max = TC.bar_compensated(e_p[k], e_t[k], k)
        f_med, f_max = TC.factors_compensated(k)
        missed |= not ok
        worst = max(worst, r_med / f_med, r_max / f_max)
    assert missed == (worst > 1.0)
    return worst


@pytest.mark.parametrize("name,inputs", TC.F32_COMPENSATED_SETS, ids=[n for n, _ in TC.F32_COMPENSATED_SETS])
def test_the_second_bar_sees_a_lost_compensation(name, inputs):
    """Two planted defects, judged with the bar's own function on the outputs the GPU case gets, against either compensated
    twin: (i) the compensation dropped (the plain float32 statement, which the first bar passes by construction); (ii) base +
    offset with the fold's residue thrown away.  Each misses at 1 500, 1e5 and 1e6 steps; a compensated statement judged
    against the other one meets the bar."""
    s = inputs()
    margins = {(d, t): _margin(s[d], s[t], s["truth"]) for d in ("twin", "base_offset_no_residue") for t in TC.COMPENSATED}
    clean = max(_margin(s["kahan"], s["base_offset"], s["truth"]), _margin(s["base_offset"], s["kahan"], s["truth"]))
    print(f"\nplanted-f32 | {name} | margin over the second bar (1 = at the bar) | "
          + " | ".join(f"{'plain' if d == 'twin' else 'no residue'} against {t} {m:.1f}" for (d, t), m in margins.items())
          + f" | one compensated statement against the other {clean:.2f}")
    assert min(margins.values()) > 1.0 and clean <= 1.0


# ---- float32 chains: three spans, the middle one shorter than a fold ------------------------------------------------------------
CHAIN3_IDS = [n for n, _ in TC.CHAIN3_F32_SETS]


@pytest.mark.parametrize("name,inputs", TC.CHAIN3_F32_SETS, ids=CHAIN3_IDS)
def test_float32_chain_twins_are_float32(name, inputs):
    """Every float32 statement of the chain comes back as complex64 (the boundary's float64 arithmetic does not leak into the
    state), and the plain one is within the float32 tolerance of record of the 80-bit run on every output."""
    s = inputs()
    for kind in ("twin",) + TC.COMPENSATED + ("base_offset_no_residue", "kahan_lost", "base_offset_lost"):
        assert s[kind]["a_end"].dtype == np.complex64 and s[kind]["rows"].dtype == np.complex64, kind
    e = TC.errors(s["twin"], s["truth"])
    print(f"\ntwin | {name} | " + " | ".join(f"{k} median {np.median(v):.2e} max {v.max():.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v.max() < H.RTOL_F32, k


@pytest.mark.parametrize("name,inputs", TC.CHAIN3_F32_SETS, ids=CHAIN3_IDS)
def test_spread_of_the_compensated_chain_statements(name, inputs):
    """test_spread_of_the_compensated_statements on the chains, rows included: the factors set on the sweeps hold on these
    seeds (every ratio within a third of its factor), so the chains are judged by the sweeps' factors, unchanged."""
    s = inputs()
    e_k, e_b = _every_output(s["kahan"], s["truth"]), _every_output(s["base_offset"], s["truth"])
    assert "rows" in e_k and "p_end" in e_k
    ratio = {k: (max(np.median(e_k[k]) / np.median(e_b[k]), np.median(e_b[k]) / np.median(e_k[k])),
                 max(e_k[k].max() / e_b[k].max(), e_b[k].max() / e_k[k].max())) for k in e_k}
    print(f"\nspread-f32 | {name} | " + " | ".join(
        f"{k} kahan {np.median(e_k[k]):.2e} {e_k[k].max():.2e} base+offset {np.median(e_b[k]):.2e} {e_b[k].max():.2e} ratio "
        f"{ratio[k][0]:.4f} {ratio[k][1]:.4f}" for k in e_k))
    for k, (r_med, r_max) in ratio.items():
        f_med, f_max = TC.factors_compensated(k)
        assert r_med <= f_med / 3 and r_max <= f_max / 3, k


@pytest.mark.parametrize("name,inputs", TC.CHAIN3_F32_SETS, ids=CHAIN3_IDS)
def test_the_second_bar_sees_a_compensation_lost_at_a_boundary(name, inputs):
    """The defect a chain can have and a sweep cannot: the compensated state kept through span 0 and lost from the first
    boundary on (the plain update in spans 1 and 2), judged as the GPU case judges, against either compensated twin.  It misses
    the second bar, as the fully plain chain does; one compensated statement against the other meets it.  base + offset without
    the fold's residue is printed and NOT asserted: over three short spans -- 28, 0 and 64 folds -- it sits at the bar."""
    s = inputs()
    lost = {(d, t): _margin(s[d + "_lost"], s[t], s["truth"]) for d in TC.COMPENSATED for t in TC.COMPENSATED}
    plain = {t: _margin(s["twin"], s[t], s["truth"]) for t in TC.COMPENSATED}
    no_residue = {t: _margin(s["base_offset_no_residue"], s[t], s["truth"]) for t in TC.COMPENSATED}
    clean = max(_margin(s["kahan"], s["base_offset"], s["truth"]), _margin(s["base_offset"], s["kahan"], s["truth"]))
    print(f"\nplanted-f32 | {name} | margin over the second bar (1 = at the bar) | "
          + " | ".join(f"{d} lost after span 0 against {t} {m:.1f}" for (d, t), m in lost.items())
          + " | " + " | ".join(f"plain against {t} {m:.1f}" for t, m in plain.items())
          + " | " + " | ".join(f"no residue against {t} {m:.2f} (not asserted: at the bar)" for t, m in no_residue.items())
          + f" | one compensated statement against the other {clean:.2f}")
    assert min(lost.values()) > 1.0 and min(plain.values()) > 1.0 and clean <= 1.0


def test_a_carried_phase_factor_takes_the_signal_power_over_the_second_bar():
    """Whose error the finding of test_gpu_truth.test_chain_of_three_spans_float32 is, decided without a GPU.  On the four-wave
    general chain the float32 kernels' wave 2 power alone (p_end / p_max of the trajectory launch) misses the second bar at its
    maximum, at ONE point, whose last span is nearly phase-matched and takes the signal towards the pumps (the report line
    printed here and by the GPU case names the point, its mismatch and the signal's size).  The Kahan chain restated in NumPy
    with cos / sin at every stage is one more compensated statement and meets the bar against the compiled one on every
    output; the same statement with ONE change -- the phase factor seeded every 16 steps and rotated once per half step between
    the seeds, as psa_rk4_kernel.inc.h has it -- misses it on p_end and p_max and on nothing else, at the kernels' point and
    with the kernels' figures (maxima 2.5e-7 and 2.2e-7 here, the scalar kernel 2.65e-7 and 2.28e-7, the packed one 2.99e-7 and
    2.57e-7; without the carried factor 4.0e-8 and 2.5e-8), the error growing inside the last span and not arriving over its
    boundary.  The compensated state and the chain's boundaries are the same in both runs: neither is involved."""
    s = TC.chain3_f32(4, False)
    e_t = _every_output(s["kahan"], s["truth"])
    verdict, worst = {}, {}
    for carried in (False, True):
        res = TC.chain3_f32_kahan_np(carried)
        e = _every_output(res, s["truth"])
        verdict[carried] = {k: TC.bar_compensated(e[k], e_t[k], k) for k in e}
        worst[carried] = int(np.argmax(e["p_max"]))
        tag = "with the carried phase factor" if carried else "with cos / sin at every stage"
        print(f"\nplanted-f32 | chain3_f32-general | NumPy Kahan chain {tag} against the kahan twin | "
              + " | ".join(f"{k} median {np.median(e[k]):.2e} max {e[k].max():.2e} ratio {r_med:.2f} {r_max:.2f}{'' if ok else ' MISSES'}"
                           for k, (ok, r_med, r_max) in verdict[carried].items()))
        print(f"planted-f32 | chain3_f32-general | NumPy Kahan chain {tag} | "
              + TC.chain3_signal_report(res["p_wave_end"][:, 2], res["p_wave_max"][:, 2], res["rows"], s))
    assert all(ok for ok, _, _ in verdict[False].values())
    assert {k for k, (ok, _, _) in verdict[True].items() if not ok} == {"p_end", "p_max"}
    assert worst[True] == int(np.argmax(e_t["p_max"]))        # the point where the compensated twins are worst as well


def test_the_carried_factor_mark_accepts_the_signal_power_alone():
    """The strict xfails of test_gpu_truth.test_chain_of_three_spans_float32 expect BarMissed, and check_float32 must let it carry
    wave 2's p_end / p_max of the trajectory launch and nothing else.  The function itself, fed CPU runs in the place of the two
    launches: the chain with the carried factor planted in both raises BarMissed naming those two outputs; the same with a
    per-wave launch that lost its compensation at the first boundary -- the defect the mark must not hide -- fails with a plain
    AssertionError; a clean compensated chain passes."""
    import test_gpu_truth as G
    s = TC.chain3_f32(4, False)
    budget = TC.chain3_f32_coupling_drift(4, False, G.CARRIED_BUDGET_F32)
    fine = np.full(TC.N, -1)

    def run(name, rows, waves):
        G.check_float32("check_float32 on CPU runs", name, dict(waves, rows=None, first_bad_step=fine), s, "kahan", known=G.SIGNAL_POWER,
                        budget=budget, plain_launch=dict(a_end=rows["a_end"], p_end=rows["p_wave_end"][:, 2], p_max=rows["p_wave_max"][:, 2],
                                                         traj=rows["rows"], first_bad_step=fine))

    carried = TC.chain3_f32_kahan_np(True)
    with pytest.raises(G.BarMissed) as hit:
        run("carried factor in both launches", carried, carried)
    assert [line.split(":")[0] for line in str(hit.value).split("\n")] == ["p_end", "p_max"]
    with pytest.raises(AssertionError) as hit:
        run("per-wave launch without its compensation", carried, s["kahan_lost"])
    assert not isinstance(hit.value, G.BarMissed) and "per-wave launch" in str(hit.value)
    run("clean", s["base_offset"], s["base_offset"])


def test_pump_power_errors_are_errors_of_the_pump_columns():
    """truth_cases.pump_power_errors, which the one-lane chain cases use to hold the pumps' powers to the bar where the signal's
    may use the frame's band, scales as truth_cases.errors does: on the float64 chain twin with the sidebands' powers replaced
    by the yardstick's, where the pumps alone carry errors' figure, the two are equal; on the twin itself it is no larger."""
    s = TC.chain3(4, False)
    twin, truth = s["twin"], s["truth"]
    pumps_only = dict(twin)
    for key in ("p_wave_end", "p_wave_max"):
        pumps_only[key] = np.concatenate([T.ld(twin[key][:, :2]), truth[key][:, 2:]], axis=1)
    e_all, e_pumps_only, e = TC.errors(twin, truth), TC.errors(pumps_only, truth), TC.pump_power_errors(twin, truth)
    for key in e:
        assert np.array_equal(e[key], e_pumps_only[key]) and (e[key] <= e_all[key]).all() and e[key].max() > 0, key


# ---- the 1e5-step float64 sets -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,inputs", TC.LONG_F64_SETS, ids=[n for n, _ in TC.LONG_F64_SETS])
def test_long_sets_are_conditioned(name, inputs):
    """e_twin of the 1e5-step GPU cases: the C double run against the C 80-bit run, below TWIN_CONDITION on every output, so
    that a ratio of errors means something."""
    s = inputs()
    assert s["truth"]["a_end"].dtype == np.clongdouble and s["twin"]["a_end"].dtype == np.complex128
    e = TC.errors(s["twin"], s["truth"])
    print(f"\ntwin | {name} | " + " | ".join(f"{k} median {np.median(v):.2e} max {v.max():.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v.max() < TC.TWIN_CONDITION, k
