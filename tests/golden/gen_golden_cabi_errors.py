#!/usr/bin/env python3
"""Writes tests/golden/cabi_errors.json: what every sweep-family entry point of libpsa_hip.so answers to a table of invalid
calls -- {"<symbol>:<case>": [return code, psa_last_error() text]} -- plus the empty (n_points == 0) calls that return 0.

The table (CASES) is what tests/test_cabi_errors.py replays against the library under test; the answers are RECORDED from the
library given on the command line, so that a change of the host code can be held to the build before it:

  python tests/golden/gen_golden_cabi_errors.py <path to the libpsa_hip.so to record>     (sets PSA_HIP_LIB)

Every call carries dummy non-NULL host pointers and is rejected by validation (or is empty): nothing reaches a device, and the
recorder refuses a table entry that got as far as looking for one (PSA_E_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cabi_errors.json")

_BUF = np.zeros(64)
P = _BUF.ctypes.data_as(C.c_void_p)                      # a dummy non-NULL buffer
_STEPS, _LENS = np.array([10, 20], np.int64), np.array([1.0, 2.0])
NAN, INF = float("nan"), float("inf")
# flags (include/psa_rk4.h)
CHECK_NAN, LDS, BLOCK64, F32_SCALAR, F32_PACKED, SPLIT, ONE_LANE, TRAJ_LD, QUAD = (1 << b for b in (8, 10, 11, 12, 13, 15, 16, 17, 18))
MAX_POINTS = 2**31 - 256

# argument lists (after device | stream) and a valid call of each family: 8 points, 4 waves (3 pairs), dummy buffers
SWEEP = dict(n_waves=4, n_points=8, n_steps=10, z_max=1.0, save_every=1, dbeta=P, dbeta2=None, gamma=P, alpha=P, a0=P,
             flags=0, a_end=P, p_end=P, p_max=P, first_bad=P, traj=None)
CHAIN = dict(n_waves=4, n_points=8, n_segments=2, n_steps=_STEPS, seg_len=_LENS, save_every=10, dbeta=P, dbeta2=None, gamma=P,
             alpha=P, a0=P, transfer=None, flags=0, a_end=P, p_end=P, p_max=P, first_bad=P, traj=None)
RK45 = dict(n_waves=4, n_points=8, z_max=1.0, rtol=1e-8, atol=1e-12, h_max=INF, first_step=0.0, max_steps=1000, n_out=0,
            dbeta=P, dbeta2=None, gamma=P, alpha=P, a0=P, flags=0, a_end=P, p_end=P, p_max=P, status=P, z_end=P,
            n_accepted=P, n_rejected=P, traj=None)
PAIRS = dict(n_pairs=3, n_points=8, n_steps=10, z_max=1.0, save_every=1, dbeta=P, gamma=P, alpha=P, a0=P, flags=0, a_end=P,
             p_wave_end=P, p_wave_max=P, first_bad=P)
WAVES = dict(p_wave_end=P, p_wave_max=P)
SP_CHAIN = dict(n_points=8, n_segments=2, n_steps=_STEPS, seg_len=_LENS, save_every=5, dbeta=P, gamma=P, alpha=P, a0=P,
                transfer=None, flags=0, a_end=P, p_wave_end=P, p_wave_max=P, first_bad=P, traj=None)
BCAST_ALL, CHECKS, LOSSLESS = 0b1111, 3 << 8, 1 << 14
# the three wave-summary families: the single-pump and multi-line sweeps, and the multi-channel and multi-line chains
SINGLE_PUMP = dict(n_points=8, n_steps=10, z_max=1.0, save_every=1, dbeta=P, gamma=P, alpha=P, a0=P, flags=0, a_end=P,
                   p_wave_end=P, p_wave_max=P, first_bad=P, traj=None)
COMB = dict(n_lines=5, **{("kappa" if k == "dbeta" else k): v for k, v in SINGLE_PUMP.items()})
PAIRS_CHAIN = dict(n_pairs=3, **SP_CHAIN)
COMB_CHAIN = dict(n_lines=5, **{("kappa" if k == "dbeta" else k): v for k, v in SP_CHAIN.items()})
REFUSED_BITS = (("one_lane", ONE_LANE), ("split", SPLIT), ("quad", QUAD), ("f32_scalar", F32_SCALAR), ("f32_packed", F32_PACKED),
                ("lds", LDS), ("bit19", 1 << 19), ("bit30", 1 << 30))


def _entry(base, *, dev, tail=None, dev_tail=None):
    """-> the ordered default arguments of one face of a family."""
    if dev:
        return dict(stream=None, **base, **(tail or {}), **(dev_tail or {}))
    return dict(device=0, **base, elapsed_ms=None, **(tail or {}))


def _nulls(names):
    return {f"null_{n}": {n: None} for n in names}


def _empty(base):
    """The n_points == 0 call with every buffer NULL."""
    return dict({k: None for k, v in base.items() if v is P}, n_points=0)


def _common(f32=False, grid=True):
    """One call per rule of the sweeps' shared validator, in its order; grid=False: a family without n_steps / save_every."""
    c = {"n_waves_5": dict(n_waves=5), "n_points_negative": dict(n_points=-1), "n_points_launch_limit": dict(n_points=MAX_POINTS + 1),
         "z_max_zero": dict(z_max=0.0), "z_max_nan": dict(z_max=NAN), "z_max_inf": dict(z_max=INF),
         "six_waves_without_dbeta2": dict(n_waves=6), "four_waves_with_dbeta2": dict(dbeta2=P),
         "traj_launch_limit": dict(traj=P, n_points=2**28 if f32 else 2**27),
         "two:n_waves_5+z_max_zero": dict(n_waves=5, z_max=0.0), "two:n_points_negative+null_dbeta": dict(n_points=-1, dbeta=None),
         "two:dbeta2+null_a0": dict(dbeta2=P, a0=None)}
    c.update(_nulls(["dbeta", "gamma", "alpha", "a0", "a_end", "p_end", "p_max"]))
    if grid:
        c.update({"n_steps_zero": dict(n_steps=0), "n_steps_2^31": dict(n_steps=2**31), "save_every_zero": dict(save_every=0),
                  "save_every_negative": dict(save_every=-3), "layouts_exclude": dict(flags=SPLIT | ONE_LANE),
                  "quad_with_one_lane": dict(flags=QUAD | ONE_LANE), "quad_with_six_waves": dict(flags=QUAD, n_waves=6, dbeta2=P),
                  "f32_scalar_and_packed": dict(flags=F32_SCALAR | F32_PACKED), "null_first_bad": dict(first_bad=None),
                  "traj_two_lane_limit": dict(traj=P, flags=SPLIT, n_points=2**27 if f32 else 2**26),
                  "traj_two_lane_limit_padded": dict(traj=P, flags=QUAD | TRAJ_LD, n_points=2**27 if f32 else 2**26),
                  "two:n_waves_5+n_steps_zero": dict(n_waves=5, n_steps=0), "two:n_steps_zero+z_max_nan": dict(n_steps=0, z_max=NAN),
                  "two:z_max_zero+save_every_zero": dict(z_max=0.0, save_every=0),
                  "two:null_gamma+layouts_exclude": dict(gamma=None, flags=SPLIT | ONE_LANE),
                  "two:save_every_zero+six_waves_without_dbeta2": dict(save_every=0, n_waves=6)})
    return c


def _sweep_cases(f32, waves):
    c = _common(f32)
    c["empty"] = _empty(SWEEP)
    c["empty_with_bad_n_steps"] = dict(_empty(SWEEP), n_steps=0)
    if waves:
        c.update({"waves_with_traj": dict(traj=P), "waves_lds_staging": dict(flags=LDS), "waves_block64": dict(flags=BLOCK64),
                  "null_p_wave_end": dict(p_wave_end=None), "null_p_wave_max": dict(p_wave_max=None),
                  "two:waves_with_traj+block64": dict(traj=P, flags=BLOCK64), "two:waves_lds_staging+n_waves_5": dict(flags=LDS, n_waves=5),
                  "two:null_p_wave_end+n_steps_zero": dict(p_wave_end=None, n_steps=0),
                  "empty": dict(_empty(SWEEP), p_wave_end=None, p_wave_max=None),
                  "empty_with_traj": dict(_empty(SWEEP), p_wave_end=None, p_wave_max=None, traj=P)})
    return c


def _chain_cases(f32, dev):
    arr = lambda a, dt: np.array(a, dt)  # noqa: E731
    c = _common(f32)
    del c["n_steps_zero"], c["n_steps_2^31"], c["two:n_waves_5+n_steps_zero"], c["two:n_steps_zero+z_max_nan"]
    for k in ("z_max_zero", "z_max_nan", "z_max_inf", "two:n_waves_5+z_max_zero", "two:z_max_zero+save_every_zero"):
        c[k] = {("seg_len" if n == "z_max" else n): (arr([v, 2.0], float) if n == "z_max" else v) for n, v in c[k].items()}
    c.update({"n_segments_zero": dict(n_segments=0), "null_n_steps": dict(n_steps=None), "null_seg_len": dict(seg_len=None),
              "first_span_n_steps_zero": dict(n_steps=arr([0, 20], np.int64)), "second_span_n_steps_zero": dict(n_steps=arr([10, 0], np.int64)),
              "second_span_n_steps_2^31": dict(n_steps=arr([10, 2**31], np.int64)), "second_span_seg_len_nan": dict(seg_len=arr([1.0, NAN], float)),
              "second_span_seg_len_zero": dict(seg_len=arr([1.0, 0.0], float)), "not_a_multiple_of_save_every": dict(n_steps=arr([10, 25], np.int64)),
              "p_wave_end_alone": dict(p_wave_end=P), "p_wave_max_alone": dict(p_wave_max=P),
              "waves_with_traj": dict(traj=P, **WAVES), "waves_lds_staging": dict(flags=LDS, **WAVES), "waves_block64": dict(flags=BLOCK64, **WAVES),
              "two:n_segments_zero+n_waves_5": dict(n_segments=0, n_waves=5), "two:null_seg_len+n_points_negative": dict(seg_len=None, n_points=-1),
              "two:not_a_multiple+p_wave_end_alone": dict(n_steps=arr([10, 25], np.int64), p_wave_end=P),
              "two:second_span_seg_len_nan+null_p_end": dict(seg_len=arr([1.0, NAN], float), p_end=None),
              "two:waves_block64+first_span_n_steps_zero": dict(flags=BLOCK64, n_steps=arr([0, 20], np.int64), **WAVES),
              "empty": _empty(CHAIN), "empty_with_waves_and_traj": dict(_empty(CHAIN), traj=P, **WAVES)})
    if dev:   # rejected after validation and before the first launch
        c["two_spans_without_workspace"] = dict(d_workspace=None)
    return c


def _single_pump_chain_cases(dev):
    """The calls of tests/test_single_pump_chain_host.py (every argument error, the flags and the workspace of the two forms)."""
    arr = lambda a, dt: np.array(a, dt)  # noqa: E731
    steps, lens = (lambda *a: dict(n_steps=arr(a, np.int64))), (lambda *a: dict(seg_len=arr(a, float)))
    null = dict(dbeta=None) if dev else dict(p_wave_max=None)
    ok = BCAST_ALL | CHECKS | LOSSLESS | BLOCK64
    c = {"n_segments_zero": dict(n_segments=0), "n_segments_negative": dict(n_segments=-1), "null_n_steps": dict(n_steps=None),
         "null_seg_len": dict(seg_len=None), "n_points_negative": dict(n_points=-1), "n_points_launch_limit": dict(n_points=MAX_POINTS + 1),
         "first_span_n_steps_zero": steps(0, 20), "second_span_n_steps_zero": steps(10, 0), "second_span_n_steps_2^31": steps(10, 5 * 2**29),
         "save_every_zero": dict(save_every=0), "second_span_not_a_multiple": steps(10, 21), "first_span_not_a_multiple": steps(11, 20),
         "null_buffer": null, "two:n_segments_zero+n_points_negative": dict(n_segments=0, n_points=-1),
         "two:n_points_negative+flag+null": dict(n_points=-1, flags=ONE_LANE, **null), "two:flag+null": dict(flags=ONE_LANE, **null),
         "two:null+not_a_multiple": dict(null, **steps(10, 21)), "traj_launch_limit": dict(n_points=2**28, traj=P),
         "no_traj_at_the_limit": dict(null, n_points=2**28), "traj_below_the_limit": dict(null, n_points=2**28 - 1, traj=P),
         "every_accepted_flag": dict(null, flags=ok | (TRAJ_LD if dev else 0)),
         "empty": dict(n_points=0)}
    for name, bad in (("zero", 0.0), ("negative", -1.0), ("inf", INF), ("nan", NAN)):
        c[f"first_span_seg_len_{name}"], c[f"second_span_seg_len_{name}"] = lens(bad, 2.0), lens(1.0, bad)
    for name, bit in (("one_lane", ONE_LANE), ("split", SPLIT), ("quad", QUAD), ("f32_scalar", F32_SCALAR), ("f32_packed", F32_PACKED),
                      ("lds", LDS), ("bit19", 1 << 19), ("bit30", 1 << 30)):
        c[f"flag_{name}"] = dict(flags=bit | CHECK_NAN)
    if dev:   # rejected after validation and before the first launch
        c.update({"two_spans_without_workspace": dict(d_workspace=None), "empty_without_workspace": dict(n_points=0, d_workspace=None)})
    else:     # the padded leading dimension belongs to the device form
        c.update({"host_traj_ld": dict(flags=TRAJ_LD), "host_traj_ld_with_traj": dict(flags=TRAJ_LD, traj=P)})
    return c


def _rk45_cases():
    c = _common(grid=False)
    c.update(_nulls(["status", "z_end", "n_accepted", "n_rejected"]))
    c.update({"flag_check_nan": dict(flags=CHECK_NAN), "flag_one_lane": dict(flags=ONE_LANE), "rtol_zero": dict(rtol=0.0),
              "rtol_below_100_eps": dict(rtol=1e-14), "rtol_nan": dict(rtol=NAN), "rtol_inf": dict(rtol=INF), "atol_zero": dict(atol=0.0),
              "atol_inf": dict(atol=INF), "h_max_zero": dict(h_max=0.0), "h_max_nan": dict(h_max=NAN), "first_step_negative": dict(first_step=-1.0),
              "first_step_inf": dict(first_step=INF), "max_steps_zero": dict(max_steps=0), "n_out_negative": dict(n_out=-1),
              "dense_output_too_large": dict(traj=P, n_out=2**60),
              "two:n_waves_5+rtol_zero": dict(n_waves=5, rtol=0.0), "two:flag_check_nan+rtol_zero": dict(flags=CHECK_NAN, rtol=0.0),
              "two:null_status+flag_one_lane": dict(status=None, flags=ONE_LANE), "two:atol_zero+null_z_end": dict(atol=0.0, z_end=None),
              "two:max_steps_zero+n_out_negative": dict(max_steps=0, n_out=-1),
              "empty": _empty(RK45), "empty_with_rtol_zero": dict(_empty(RK45), rtol=0.0)})
    return c


def _pairs_cases():
    c = {"n_pairs_zero": dict(n_pairs=0), "n_pairs_17": dict(n_pairs=17), "n_points_negative": dict(n_points=-1),
         "launch_limit_16_lanes": dict(n_pairs=16, n_points=2**31), "launch_limit_2_lanes": dict(n_pairs=1, n_points=MAX_POINTS + 1),
         "launch_limit_4_lanes": dict(n_points=MAX_POINTS // 2 + 1), "n_steps_zero": dict(n_steps=0), "n_steps_2^31": dict(n_steps=2**31),
         "z_max_zero": dict(z_max=0.0), "z_max_nan": dict(z_max=NAN), "z_max_inf": dict(z_max=INF), "save_every_zero": dict(save_every=0),
         "flag_one_lane": dict(flags=ONE_LANE | CHECK_NAN), "flag_traj_ld": dict(flags=TRAJ_LD), "flag_unknown": dict(flags=1 << 30),
         "two:n_pairs_zero+n_points_negative": dict(n_pairs=0, n_points=-1), "two:n_steps_zero+save_every_zero": dict(n_steps=0, save_every=0),
         "two:flag_one_lane+null_dbeta": dict(flags=ONE_LANE, dbeta=None), "two:launch_limit+z_max_nan": dict(n_pairs=16, n_points=2**31, z_max=NAN),
         "empty": _empty(PAIRS), "empty_with_flag_one_lane": dict(_empty(PAIRS), flags=ONE_LANE)}
    c.update(_nulls([k for k, v in PAIRS.items() if v is P]))
    return c


def _wave_family_cases(base, dev, count=None):
    """One call per rule of a wave-summary family's validator, in its order: the single-pump and multi-line sweeps, and the
    multi-channel and multi-line chains (``base`` with n_segments).  count: (argument, below, above) of n_pairs / n_lines."""
    arr = lambda a, dt: np.array(a, dt)  # noqa: E731
    chain, pairs = "n_segments" in base, "n_pairs" in base
    steps, lens = (lambda *a: dict(n_steps=arr(a, np.int64))), (lambda *a: dict(seg_len=arr(a, float)))
    mismatch = "kappa" if "kappa" in base else "dbeta"
    null = {mismatch: None} if dev else dict(p_wave_max=None)
    ok = (BCAST_ALL if chain else 0b0111) | CHECKS | LOSSLESS | BLOCK64
    c = {}
    if chain:
        c.update({"n_segments_zero": dict(n_segments=0), "n_segments_negative": dict(n_segments=-1), "null_n_steps": dict(n_steps=None),
                  "null_seg_len": dict(seg_len=None)})
    if count:
        name, low, high = count
        c.update({f"{name}_{low}": {name: low}, f"{name}_{high}": {name: high}})
    c["n_points_negative"] = dict(n_points=-1)
    if pairs:
        c.update({"launch_limit_2_lanes": dict(n_pairs=1, n_points=MAX_POINTS + 1), "launch_limit_4_lanes": dict(n_points=MAX_POINTS // 2 + 1),
                  "launch_limit_16_lanes": dict(n_pairs=16, n_points=2**31)})
    else:
        c["n_points_launch_limit"] = dict(n_points=MAX_POINTS + 1)
    if chain:
        c.update({"first_span_n_steps_zero": steps(0, 20), "first_span_n_steps_2^31": steps(5 * 2**29, 20),
                  "second_span_n_steps_zero": steps(10, 0), "second_span_n_steps_2^31": steps(10, 5 * 2**29)})
        for name, bad in (("zero", 0.0), ("negative", -1.0), ("inf", INF), ("nan", NAN)):
            c[f"first_span_seg_len_{name}"], c[f"second_span_seg_len_{name}"] = lens(bad, 2.0), lens(1.0, bad)
    else:
        c.update({"n_steps_zero": dict(n_steps=0), "n_steps_2^31": dict(n_steps=2**31), "z_max_zero": dict(z_max=0.0),
                  "z_max_negative": dict(z_max=-1.0), "z_max_nan": dict(z_max=NAN), "z_max_inf": dict(z_max=INF)})
    c["save_every_zero"] = dict(save_every=0)
    for name, bit in REFUSED_BITS:
        c[f"flag_{name}"] = dict(flags=bit | CHECK_NAN)
    if not chain:   # the chain's own bit
        c["flag_bcast_transfer"] = dict(flags=1 << 3)
    if dev:         # accepted: the call fails at a later rule
        c.update({"dev_traj_ld_then_null": dict(null, flags=TRAJ_LD), "dev_traj_ld_with_traj_then_null": dict(null, flags=TRAJ_LD, traj=P)})
    else:           # the padded leading dimension belongs to the device form
        c.update({"host_traj_ld": dict(flags=TRAJ_LD), "host_traj_ld_with_traj": dict(flags=TRAJ_LD, traj=P)})
    c["every_accepted_flag"] = dict(null, flags=ok | (TRAJ_LD if dev else 0))
    c.update(_nulls([k for k, v in base.items() if v is P]))
    # the row bound: refused at 2^28 points with rows, not one point below it, and not without rows
    c["traj_launch_limit"] = dict(n_points=2**28, traj=P)
    if dev:
        c["traj_launch_limit_padded"] = dict(n_points=2**28, traj=P, flags=TRAJ_LD)
    later = steps(10, 21) if chain else null   # a chain has rules after the row bound; a sweep is stopped in front of it
    c.update({"traj_below_the_limit": dict(later, n_points=2**28 - 1, traj=P), "no_traj_at_the_limit": dict(later, n_points=2**28)})
    if chain:
        c.update({"first_span_not_a_multiple": steps(11, 20), "second_span_not_a_multiple": steps(10, 21),
                  "two:n_segments_zero+n_points_negative": dict(n_segments=0, n_points=-1),
                  "two:null+not_a_multiple": dict(null, **steps(10, 21)),
                  "two:traj_launch_limit+not_a_multiple": dict(n_points=2**28, traj=P, **steps(10, 21))})
        if not pairs:   # one span of the multi-channel chain is the sweep's trajectory form, which may end behind its last row
            c["one_span_not_a_multiple"] = dict(n_segments=1, **steps(11, 20))
        if dev:   # rejected after validation and before the first launch
            c.update({"two_spans_without_workspace": dict(d_workspace=None), "empty_without_workspace": dict(n_points=0, d_workspace=None)})
    if count:
        name, low, _ = count
        c[f"two:{name}+n_points_negative"] = {name: low, "n_points": -1}
        c[f"two:{name}+flag+null"] = dict(null, flags=ONE_LANE, **{name: low})
        if chain:
            c[f"two:null_n_steps+{name}"] = {"n_steps": None, name: low}
    c.update({"two:n_points_negative+save_every_zero": dict(n_points=-1, save_every=0),
              "two:save_every_zero+flag": dict(save_every=0, flags=ONE_LANE), "two:flag+null": dict(flags=ONE_LANE, **null),
              "two:null+traj_launch_limit": dict(null, n_points=2**28, traj=P),
              "empty": _empty(base), "empty_with_traj": dict(_empty(base), traj=P),
              "empty_with_refused_flag": dict(_empty(base), flags=ONE_LANE)})
    return c


def cases() -> dict:
    """{symbol: (default arguments in call order, {case: overrides})} for every sweep-family entry point, both faces."""
    out = {}
    for t in ("f64", "f32"):
        f32 = t == "f32"
        for dev in (False, True):
            sfx = "_dev" if dev else ""
            out[f"psa_rk4_sweep_{t}{sfx}"] = (_entry(SWEEP, dev=dev), _sweep_cases(f32, False))
            out[f"psa_rk4_sweep_waves_{t}{sfx}"] = (_entry(SWEEP, dev=dev, tail=WAVES), _sweep_cases(f32, True))
            out[f"psa_rk4_chain_{t}{sfx}"] = (_entry(CHAIN, dev=dev, tail=dict(p_wave_end=None, p_wave_max=None),
                                                     dev_tail=dict(d_workspace=P)), _chain_cases(f32, dev))
    for dev in (False, True):
        sfx = "_dev" if dev else ""
        out[f"psa_rk45_sweep_f64{sfx}"] = (_entry(RK45, dev=dev), _rk45_cases())
        out[f"psa_rk4_sweep_pairs_f64{sfx}"] = (_entry(PAIRS, dev=dev), _pairs_cases())
        out[f"psa_rk4_single_pump_chain_f64{sfx}"] = (_entry(SP_CHAIN, dev=dev, dev_tail=dict(d_workspace=P)),
                                                      _single_pump_chain_cases(dev))
        ws = dict(d_workspace=P)
        out[f"psa_rk4_pairs_chain_f64{sfx}"] = (_entry(PAIRS_CHAIN, dev=dev, dev_tail=ws),
                                                _wave_family_cases(PAIRS_CHAIN, dev, ("n_pairs", 0, 17)))
        out[f"psa_rk4_comb_chain_f64{sfx}"] = (_entry(COMB_CHAIN, dev=dev, dev_tail=ws),
                                               _wave_family_cases(COMB_CHAIN, dev, ("n_lines", 2, 13)))
        for t in ("f64", "f32"):   # both precisions share one validator and one row bound: "below 2^28 points"
            out[f"psa_rk4_single_pump_{t}{sfx}"] = (_entry(SINGLE_PUMP, dev=dev), _wave_family_cases(SINGLE_PUMP, dev))
            out[f"psa_rk4_comb_{t}{sfx}"] = (_entry(COMB, dev=dev), _wave_family_cases(COMB, dev, ("n_lines", 2, 13)))
    return out


def _arg(v):
    return v.ctypes.data_as(C.c_void_p) if isinstance(v, np.ndarray) else v


def replay(lib, symbol: str) -> dict:
    """{"<symbol>:<case>": [rc, message]} of every case of one entry point against ``lib`` (a bound ctypes library)."""
    base, table = cases()[symbol]
    fn, got = getattr(lib, symbol), {}
    for name, over in table.items():
        assert set(over) <= set(base), (symbol, name, set(over) - set(base))
        rc = int(fn(*[_arg(v) for v in dict(base, **over).values()]))
        got[f"{symbol}:{name}"] = [rc, "" if rc == 0 else lib.psa_last_error().decode()]
    return got


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    os.environ["PSA_HIP_LIB"] = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import psa_amd._native as nat
    table = {}
    for symbol in cases():
        table.update(replay(nat.lib(), symbol))
    reached = [k for k, (rc, _) in table.items() if rc == -7 or rc > 0 or (rc == 0 and ":empty" not in k)]
    assert not reached, f"these calls passed validation: {reached}"
    with open(OUT, "w", encoding="utf-8") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(table[k])}" for k in sorted(table)) + "\n}\n")
    print(f"wrote {OUT}: {len(table)} calls of {len(cases())} entry points, recorded from {nat.LIB_PATH} ({nat.version()})")


if __name__ == "__main__":
    main()
