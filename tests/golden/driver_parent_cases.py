"""The cases of tests/test_driver_parent.py, shared with gen_golden_driver_parent.py (which records driver_parent.json.gz): the
twelve drivers of the single-pump, multi-channel ("pairs") and multi-line ("comb") models and of the copier - PSA scans, as
simulation.py and scan_mismtach.py behaved before they shared one driver path.

A driver reaches the device through eight functions of _native, each looked up when called, so over a stand-in of the eight
it is a pure function of its arguments: StandIn records every call (arrays as dtype, shape and bytes, scalars with their
type, the device) and returns arrays of the real wrappers' keys, dtypes and shapes, drawn from a generator seeded by a digest
of the function's name and its inputs -- never by the order of the calls, which ``devices=[0, 1]`` leaves to two threads; the
calls of a case are stored sorted by device.  A case's record is its calls and everything the driver returned, or the type and
text of what it raised."""
import dataclasses
import hashlib
import threading
from types import SimpleNamespace

import numpy as np

HOST_FUNCTIONS = ("sweep_pairs_host", "single_pump_host", "comb_host", "chain_host", "single_pump_chain_host",
                  "pairs_chain_host", "comb_chain_host", "gain_summary_host")


# ---- values as JSON: nothing rounded, nothing compared by ==  ---------------------------------------------------------------
def encode(x):
    """Arrays as dtype, shape and bytes; scalars with their type; containers in their order; a result object by its fields."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return {"a": x.dtype.str, "s": list(x.shape), "b": np.ascontiguousarray(x).tobytes().hex()}
    if isinstance(x, np.generic):
        return {"n": x.dtype.str, "b": x.tobytes().hex()}
    if isinstance(x, bool):
        return {"t": x}
    if isinstance(x, int):
        return {"i": x}
    if isinstance(x, float):
        return {"f": x.hex()}
    if isinstance(x, complex):
        return {"c": [x.real.hex(), x.imag.hex()]}
    if isinstance(x, str):
        return {"u": x}
    if isinstance(x, (type, np.dtype)):
        return {"d": np.dtype(x).str}
    if isinstance(x, tuple):
        return {"T": [encode(v) for v in x]}
    if isinstance(x, list):
        return {"L": [encode(v) for v in x]}
    if isinstance(x, dict):
        return {"D": [[str(k), encode(v)] for k, v in x.items()]}
    if dataclasses.is_dataclass(x):
        return {"R": type(x).__name__, "F": [[f.name, encode(getattr(x, f.name))] for f in dataclasses.fields(x)]}
    raise TypeError(f"no encoding for {type(x)}")


# ---- the stand-in -----------------------------------------------------------------------------------------------------------
def _digest_seed(name: str, args: dict) -> int:
    h = hashlib.sha256(name.encode())
    for k in sorted(args):
        if k != "device":
            h.update(repr((k, encode(args[k]))).encode())
    return int.from_bytes(h.digest()[:8], "little")


def gain_summary_numpy(p_metric, first_bad_step, p0_sig, gain_db=True):
    """The NaN rule of psa_gain_summary_*: a point that failed, a non-positive or non-finite seed power, a non-finite or
    non-positive ratio give NaN -> (gain in p_metric's precision, argmax, max, number of finite gains)."""
    p = np.asarray(p_metric)
    p = p.astype(np.float32 if p.dtype == np.float32 else np.float64)
    ok = np.ones(p.shape, dtype=bool) if first_bad_step is None else np.asarray(first_bad_step) < 0
    with np.errstate(all="ignore"):
        ok = ok & bool(np.isfinite(p0_sig) and p0_sig > 0.0)
        g = p.astype(np.float64) / (p0_sig if p0_sig else 1.0)
        ok &= np.isfinite(g) & (g > 0.0)
        g = np.where(ok, 10.0 * np.log10(np.where(ok, g, 1.0)) if gain_db else g, np.nan).astype(p.dtype)
    bi = int(np.nanargmax(g)) if ok.any() else -1
    return g, bi, (float(g[bi]) if bi >= 0 else float("nan")), int(ok.sum())


class StandIn:
    """The eight host functions without a device.  ``bad = (point, step)`` plants one failing point in every launch that has
    that point: first_bad_step = step and NaN in its summaries."""

    def __init__(self, bad=None):
        self.bad, self.calls, self._lock = bad, [], threading.Lock()

    def install(self, nat):
        """Put the stand-in into the module ``nat`` -> what was there, for restore()."""
        saved = {name: getattr(nat, name) for name in HOST_FUNCTIONS}
        for name in HOST_FUNCTIONS:
            setattr(nat, name, getattr(self, name))
        return saved

    @staticmethod
    def restore(nat, saved):
        for name, fn in saved.items():
            setattr(nat, name, fn)

    def sorted_calls(self):
        """The recorded calls, sorted by device (one device's calls keep their order)."""
        return [c for _, c in sorted(enumerate(self.calls), key=lambda ic: (ic[1]["device"], ic[0]))]

    def _note(self, name: str, args: dict) -> np.random.Generator:
        call = {"fn": name, "device": int(args["device"]), "args": [[k, encode(args[k])] for k in sorted(args)]}
        with self._lock:
            self.calls.append(call)
        return np.random.default_rng(_digest_seed(name, args))

    def _outputs(self, rng, N, nw, real, n_rows, *, want_traj, rows_key, scalar_summary, wave_summary):
        cplx = np.complex64 if np.dtype(real) == np.float32 else np.complex128
        draw = lambda *shape: rng.uniform(0.05, 2.0, shape).astype(real)   # noqa: E731
        out = {"a_end": (rng.normal(size=(N, nw)) + 1j * rng.normal(size=(N, nw))).astype(cplx)}
        if scalar_summary:
            out.update(p_end=draw(N), p_max=draw(N))
        out.update(p_wave_end=draw(N, nw) if wave_summary else None, p_wave_max=draw(N, nw) if wave_summary else None)
        out["first_bad_step"] = np.full(N, -1, dtype=np.int64)
        if rows_key:
            out["traj"] = (rng.normal(size=(N, n_rows, nw)) + 1j * rng.normal(size=(N, n_rows, nw))).astype(cplx) if want_traj else None
        out["elapsed_ms"] = float(rng.uniform(0.01, 1.0))
        if self.bad is not None and self.bad[0] < N:
            k = self.bad[0]
            out["first_bad_step"][k] = self.bad[1]
            for key in ("p_end", "p_max", "p_wave_end", "p_wave_max"):
                if out.get(key) is not None:
                    out[key][k] = np.nan
        return out

    def _sweep(self, name, mismatch_key, nw_of, args, rows_key):
        rng = self._note(name, args)
        mis = np.asarray(args[mismatch_key])
        if name == "single_pump_host":
            mis = np.atleast_1d(mis)
        se, n = int(args["save_every"]), int(args["n_steps"])
        return self._outputs(rng, int(mis.shape[0]), nw_of(mis), np.dtype(args.get("dtype", np.float64)),
                             n // se + 1 if se > 0 else 0, want_traj=bool(args.get("want_traj")), rows_key=rows_key,
                             scalar_summary=False, wave_summary=True)

    def sweep_pairs_host(self, dbeta, *, n_steps, z_max, save_every, gamma, alpha, a0, check_nan=True, exact_step=None, device=0,
                         extra_flags=0):
        args = dict(locals())
        del args["self"]
        return self._sweep("sweep_pairs_host", "dbeta", lambda m: 2 + 2 * int(m.shape[1]), args, False)

    def single_pump_host(self, dbeta, *, n_steps, z_max, save_every, gamma, alpha, a0, check_nan=True, exact_step=None,
                         want_traj=False, device=0, extra_flags=0, dtype=np.float64):
        args = dict(locals())
        del args["self"]
        return self._sweep("single_pump_host", "dbeta", lambda m: 3, args, True)

    def comb_host(self, kappa, *, n_steps, z_max, save_every, gamma, alpha, a0, check_nan=True, want_traj=False, device=0,
                  extra_flags=0, dtype=np.float64):
        args = dict(locals())
        del args["self"]
        return self._sweep("comb_host", "kappa", lambda m: int(m.shape[1]), args, True)

    def _chain(self, name, args, *, scalar_summary, wave_summary):
        rng = self._note(name, args)
        db = np.asarray(args["dbeta"])
        a0 = np.asarray(args["a0"])
        se, steps = int(args["save_every"]), np.asarray(args["n_steps"], dtype=np.int64)
        return self._outputs(rng, int(db.shape[1]), int(a0.shape[-1]), np.dtype(args.get("dtype", np.float64)),
                             int(np.sum(steps // se + 1)) if se > 0 else 0, want_traj=bool(args["want_traj"]), rows_key=True,
                             scalar_summary=scalar_summary, wave_summary=wave_summary)

    def chain_host(self, dbeta, *, n_steps, seg_len, save_every, gamma, alpha, a0, transfers=None, dbeta2=None, check_nan=True,
                   exact_step=None, want_traj=False, dtype=np.float64, device=0, wave_summary=False, extra_flags=0):
        args = dict(locals())
        del args["self"]
        return self._chain("chain_host", args, scalar_summary=True, wave_summary=bool(wave_summary))

    def single_pump_chain_host(self, dbeta, *, n_steps, seg_len, save_every, gamma, alpha, a0, transfers=None, check_nan=True,
                               exact_step=None, want_traj=False, device=0, extra_flags=0):
        args = dict(locals())
        del args["self"]
        return self._chain("single_pump_chain_host", args, scalar_summary=False, wave_summary=True)

    def pairs_chain_host(self, dbeta, *, n_steps, seg_len, save_every, gamma, alpha, a0, transfers=None, check_nan=True,
                         exact_step=None, want_traj=False, device=0, extra_flags=0):
        args = dict(locals())
        del args["self"]
        return self._chain("pairs_chain_host", args, scalar_summary=False, wave_summary=True)

    def comb_chain_host(self, dbeta, *, n_steps, seg_len, save_every, gamma, alpha, a0, transfers=None, check_nan=True,
                        exact_step=None, want_traj=False, device=0, extra_flags=0):
        args = dict(locals())
        del args["self"]
        return self._chain("comb_chain_host", args, scalar_summary=False, wave_summary=True)

    def gain_summary_host(self, p_metric, first_bad_step, p0_sig, *, gain_db=True, device=0):
        args = dict(locals())
        del args["self"]
        self._note("gain_summary_host", args)
        return gain_summary_numpy(p_metric, first_bad_step, float(p0_sig), bool(gain_db))


# ---- the cases --------------------------------------------------------------------------------------------------------------
C_LIGHT = 299792458.0
LAM0 = 1554e-9
W0 = 2.0 * np.pi * C_LIGHT / LAM0
BAD = (2, 7)            # the planted failure: point 2 at step 7 (the first span of a chain)
BAD_SINGLE = (0, 25)    # ... of a single run: its one point, at step 25 (span 1, local step 5 of a 20 + 30 chain)


def package(pkg):
    """The modules the cases are built from, of the package ``pkg`` (psa_amd, or a copy under another name)."""
    import importlib
    mod = lambda name: importlib.import_module(f"{pkg.__name__}.{name}")   # noqa: E731
    return SimpleNamespace(native=mod("_native"), config=mod("config"), dispersion=mod("dispersion"),
                           phase_matching=mod("phase_matching"), simulation=mod("simulation"), scans=mod("scan_mismtach"))


def _drop(d: dict, *names) -> dict:
    return {k: v for k, v in d.items() if k not in names}


def cases(P) -> dict:
    """-> {key: (driver, keyword arguments, the stand-in's planted failure or None)}, failing calls under "err/..."."""
    sim, scan = P.simulation, P.scans
    cfg = lambda n=20, **kw: P.config.custom_simulation_config(z_max=0.1 * n, dz=0.1, **kw)   # noqa: E731
    disp = lambda s=1.0, **kw: P.dispersion.DispersionParams(**{**dict(omega_ref=W0, beta2=-2.3e-28 * s, beta3=4.1e-41 * s,   # noqa: E731
                                                                       beta4=-3.2e-55 * s), **kw})
    provided = lambda v: P.phase_matching.PhaseMatchingConfig(method=P.phase_matching.PhaseMatchingMethod.PROVIDED,   # noqa: E731
                                                             provided_delta_beta=v)
    taylor = P.phase_matching.PhaseMatchingConfig(method=P.phase_matching.PhaseMatchingMethod.GENERAL_TAYLOR, max_order=4,
                                                  atol=0.0, rtol=1e-12)
    WS = W0 + 2.0 * np.pi * 1.0e12
    DW = 2.0 * np.pi * 100e9
    L1, L2 = 1540e-9, 1560e-9
    OM1, OM3 = [2.0 * np.pi * 0.5e12], [2.0 * np.pi * 0.5e12, -2.0 * np.pi * 0.9e12, 2.0 * np.pi * 1.4e12]
    P3, P5 = [1e-4, 0.4, 2e-4], [1e-5, 0.25, 0.25, 0.0, 2e-5]       # comb inputs; line 3 of the five is dark
    out = {}

    def valid(key, fn, kw, bad=None):
        assert key not in out, key
        out[key] = (fn, kw, bad)

    def failing(prefix, fn, base, singles, extra_pairs=()):
        """Every rule once, in the validator's order, then every two neighbours together: the pair's record fixes the order."""
        rules = dict(singles)
        assert len(rules) == len(singles), prefix
        for name, over in singles:
            valid(f"err/{prefix}/{name}", fn, {**base, **over})
        names = [name for name, _ in singles]
        for n1, n2 in list(zip(names, names[1:])) + list(extra_pairs):
            if not set(rules[n1]) & set(rules[n2]) and f"err/{prefix}/{n1}+{n2}" not in out:
                valid(f"err/{prefix}/{n1}+{n2}", fn, {**base, **rules[n1], **rules[n2]})

    # -- run_single_pump_simulation
    sp = dict(cfg=cfg(), gamma=1.1, alpha=1.15e-2, omega_pump=W0, omega_signal=WS, p_in=[0.4, 1e-4, 2e-6], dispersion=disp())
    sp_km = dict(sp, cfg=cfg(30), dispersion=disp(1e3), phase_in=[0.1, -0.2, 0.3], max_order=3, length_unit="km")
    f = sim.run_single_pump_simulation
    valid("run_sp/m", f, sp)
    valid("run_sp/km", f, sp_km)
    valid("run_sp/km_to_m", f, dict(sp_km, return_length_unit="m"))
    valid("run_sp/m_to_km_save5", f, dict(sp, cfg=cfg(20, save_every=5), return_length_unit="km"))
    valid("run_sp/bad_unchecked", f, dict(sp, cfg=cfg(check_nan=False)), (0, 7))
    valid("run_sp/bad", f, sp, (0, 7))
    sp_rules = [
        ("cfg", dict(cfg=P.config.custom_simulation_config(z_max=2.0, dz=-0.1))),
        ("unit", dict(length_unit="cm")),
        ("wp_nan", dict(omega_pump=float("nan"))),
        ("wp_neg", dict(omega_pump=-W0)),
        ("ws_zero", dict(omega_signal=0.0)),
        ("idler", dict(omega_signal=2.5 * W0)),
        ("p_shape", dict(p_in=[0.4, 1e-4, 2e-6, 0.0])),
        ("p_nan", dict(p_in=[0.4, float("nan"), 0.0])),
        ("p_neg", dict(p_in=[0.4, -1e-4, 0.0])),
        ("ph_shape", dict(phase_in=[0.0, 0.0])),
        ("ph_inf", dict(phase_in=[0.0, float("inf"), 0.0])),
    ]
    failing("run_sp", f, sp, sp_rules + [
        ("disp_none", dict(dispersion=None)),
        ("order_type", dict(max_order=2.0)),
        ("order_neg", dict(max_order=-1)),
        ("disp_type", dict(dispersion="smf")),
        ("save_every", dict(cfg=cfg(save_every=0))),
        ("dbeta_inf", dict(dispersion=disp(beta2=1e300))),
    ], extra_pairs=[("unit", "p_neg"), ("wp_neg", "disp_none")])
    valid("err/run_sp/return_unit", f, dict(sp, return_length_unit="mm"))

    # -- run_comb_simulation
    cb = dict(cfg=cfg(), gamma=1.1, alpha=1.15e-2, omega_center=W0, line_spacing=DW, p_in=P3, dispersion=disp())
    cb_km = dict(cb, cfg=cfg(30), dispersion=disp(1e3), p_in=P5, phase_in=[0.1, -0.2, 0.3, 0.0, 1.0], max_order=3,
                 length_unit="km")
    f = sim.run_comb_simulation
    valid("run_comb/m3", f, cb)
    valid("run_comb/km5_dark", f, cb_km)
    valid("run_comb/bad_unchecked", f, dict(cb, cfg=cfg(check_nan=False)), (0, 7))
    valid("run_comb/bad", f, cb_km, (0, 25))
    comb_rules = lambda name: [   # noqa: E731
        ("p_ndim", {name: 0.5}),
        ("p_few", {name: [0.5, 0.5]}),
        ("p_many", {name: [0.1] * 13}),
        ("p_nan", {name: [0.4, float("nan"), 0.1]}),
        ("p_neg", {name: [0.4, -0.1, 0.1]}),
        ("p_2d", {name: [P3, P3]}),
        ("ph_shape", dict(phase_in=[0.0, 0.0])),
        ("ph_nan", dict(phase_in=[0.0, float("nan"), 0.0])),
    ]
    line_rules = [
        ("wc_nan", dict(omega_center=float("nan"))),
        ("wc_neg", dict(omega_center=-W0)),
        ("dw_zero", dict(line_spacing=0.0)),
        ("dw_inf", dict(line_spacing=float("inf"))),
        ("order_type", dict(max_order=4.0)),
        ("order_low", dict(max_order=1)),
        ("lowest", dict(line_spacing=1.5 * W0)),
    ]
    failing("run_comb", f, cb, [("cfg", dict(cfg=P.config.custom_simulation_config(z_max=-1.0, dz=0.1))), ("unit", dict(length_unit="mm"))]
            + comb_rules("p_in") + [("disp_none", dict(dispersion=None)), ("disp_type", dict(dispersion=3.0))] + line_rules
            + [("kappa_inf", dict(dispersion=disp(beta2=1e300)))],
            extra_pairs=[("unit", "ph_nan"), ("p_neg", "disp_none"), ("disp_none", "lowest")])

    # -- run_concatenated_simulation (four waves)
    om4 = [W0 + DW, W0 - DW, W0 + 3 * DW, W0 - 3 * DW]
    s4 = [dict(cfg=cfg(), gamma=1.1, alpha=1.15e-2, dispersion=disp()),
          dict(cfg=cfg(30), gamma=1.3, alpha=0.0, phase_matching_cfg=provided(-0.3))]
    c4 = dict(spans=s4, omega=om4, p_in=[0.25, 0.25, 1e-4, 1e-6])
    c4_km = dict(spans=[dict(cfg=cfg(30), gamma=1.1, alpha=0.0, beta_legacy=[5.0, 5.1, 4.9, 5.3]),
                        dict(cfg=cfg(), gamma=1.2, alpha=2e-2, dispersion=disp(1e3), phase_matching_cfg=taylor),
                        dict(cfg=cfg(), gamma=1.2, alpha=2e-2, dispersion=disp(1e3))],
                 omega=om4, p_in=[0.25, 0.25, 1e-4, 1e-6], phase_in=[0.1, 0.2, -0.3, 0.0],
                 transfers=[sim.mid_stage([0.0, 0.0, -1.0, -1.0], [0.5, 0.5, 0.0, 0.0]), np.array([1.0, 1.0, 0.5j, 0.0])],
                 length_unit="km")
    f = sim.run_concatenated_simulation
    valid("cat4/m", f, c4)
    valid("cat4/one_span", f, dict(c4, spans=tuple(s4[:1]), transfers=[]))
    valid("cat4/km", f, c4_km)
    valid("cat4/km_to_m", f, dict(c4_km, return_length_unit="m"))
    valid("cat4/bad_span0", f, c4, (0, 7))
    valid("cat4/bad_span1", f, c4, BAD_SINGLE)
    valid("cat4/bad_unchecked", f, dict(c4, spans=[dict(s, cfg=cfg(20, check_nan=False)) for s in s4]), BAD_SINGLE)
    span_rules = lambda base: [   # noqa: E731  (the rules the three span loops share)
        ("unknown", dict(spans=[base[0], dict(base[1], length=3.0)])),
        ("no_cfg", dict(spans=[_drop(base[0], "cfg"), base[1]])),
        ("no_gamma", dict(spans=[base[0], _drop(base[1], "gamma")])),
        ("no_alpha_unknown", dict(spans=[dict(_drop(base[0], "alpha"), beta=1.0, zeta=2.0), base[1]])),
        ("span_cfg", dict(spans=[base[0], dict(base[1], cfg=P.config.custom_simulation_config(z_max=1.0, dz=2.0))])),
        ("span_disp_type", dict(spans=[dict(base[0], dispersion=[1.0]), base[1]])),
    ]
    end_rules = lambda base, w: [   # noqa: E731  (_run_spans)
        ("save_every", dict(spans=[base[0], dict(base[1], cfg=cfg(30, save_every=5))])),
        ("check_nan", dict(spans=[dict(base[0], cfg=cfg(20, check_nan=False)), base[1]])),
        ("tr_count", dict(transfers=[])),
        ("tr_shape", dict(transfers=[np.ones(w + 1)])),
        ("multiple", dict(spans=[dict(base[0], cfg=cfg(25)), base[1]])),
    ]
    failing("cat4", f, c4, [
        ("empty", dict(spans=[])),
        ("unit", dict(length_unit="cm")),
        ("om_shape", dict(omega=om4[:3])),
        ("om_nan", dict(omega=[W0, W0, float("nan"), W0])),
        ("om_neg", dict(omega=[W0, W0, -W0, W0])),
        ("p_shape", dict(p_in=[0.25, 0.25, 1e-4])),
        ("p_nan", dict(p_in=[0.25, float("nan"), 1e-4, 0.0])),
        ("p_neg", dict(p_in=[0.25, 0.25, -1e-4, 0.0])),
        ("ph_shape", dict(phase_in=[0.0])),
        ("ph_nan", dict(phase_in=[0.0, 0.0, float("nan"), 0.0])),
    ] + span_rules(s4) + [
        ("legacy_shape", dict(spans=[dict(cfg=cfg(), gamma=1.0, alpha=0.0, beta_legacy=[1.0, 2.0]), s4[1]])),
        ("legacy_nan", dict(spans=[dict(cfg=cfg(), gamma=1.0, alpha=0.0, beta_legacy=[1.0, 2.0, float("nan"), 1.0]), s4[1]])),
        ("neither", dict(spans=[s4[0], dict(cfg=cfg(30), gamma=1.0, alpha=0.0)])),
        ("pm_type", dict(spans=[s4[0], dict(s4[1], phase_matching_cfg="provided")])),
    ] + end_rules(s4, 4), extra_pairs=[("empty", "unit"), ("unit", "unknown"), ("ph_nan", "neither")])
    valid("err/cat4/return_unit", f, dict(c4, return_length_unit="mm"))

    # -- run_concatenated_single_pump_simulation
    s3 = [dict(cfg=cfg(), gamma=1.1, alpha=1.15e-2, dispersion=disp(), max_order=3),
          dict(cfg=cfg(30), gamma=1.3, alpha=0.0, phase_matching_cfg=provided(-0.3))]
    c3 = dict(spans=s3, omega_pump=W0, omega_signal=WS, p_in=[0.4, 1e-4, 2e-6])
    c3_km = dict(spans=[dict(cfg=cfg(30), gamma=1.1, alpha=0.0, phase_matching_cfg=provided(250.0)),
                        dict(cfg=cfg(), gamma=1.2, alpha=2e-2, dispersion=disp(1e3))],
                 omega_pump=W0, omega_signal=WS, p_in=[0.4, 1e-4, 2e-6], phase_in=[0.1, 0.2, -0.3],
                 transfers=[sim.single_pump_mid_stage([0.0, -1.0, -1.0], [0.5, 0.0, 0.0])], length_unit="km")
    f = sim.run_concatenated_single_pump_simulation
    valid("cat_sp/m", f, c3)
    valid("cat_sp/one_span", f, dict(c3, spans=tuple(s3[:1])))
    valid("cat_sp/km", f, c3_km)
    valid("cat_sp/km_to_m", f, dict(c3_km, return_length_unit="m"))
    valid("cat_sp/bad_span0", f, c3, (0, 7))
    valid("cat_sp/bad_span1", f, c3_km, (0, 31))
    valid("cat_sp/bad_unchecked", f, dict(c3, spans=[dict(s, cfg=cfg(20, check_nan=False)) for s in s3]), (0, 7))
    failing("cat_sp", f, c3, [("empty", dict(spans=()))] + sp_rules[1:] + span_rules(s3)[:4] + [
        ("both", dict(spans=[dict(s3[0], phase_matching_cfg=provided(0.0)), s3[1]])),
        ("neither", dict(spans=[s3[0], _drop(s3[1], "phase_matching_cfg")])),
        ("pm_type", dict(spans=[s3[0], dict(s3[1], phase_matching_cfg=0.3)])),
        ("pm_method", dict(spans=[s3[0], dict(s3[1], phase_matching_cfg=taylor)])),
        ("order_type", dict(spans=[dict(s3[0], max_order=2.0), s3[1]])),
        ("order_neg", dict(spans=[dict(s3[0], max_order=-2), s3[1]])),
    ] + span_rules(s3)[4:] + [("dbeta_nan", dict(spans=[dict(s3[0], dispersion=disp(beta2=1e300)), s3[1]]))] + end_rules(s3, 3),
        extra_pairs=[("empty", "unit"), ("ph_inf", "both"), ("both", "order_neg"), ("idler", "unknown")])

    # -- run_concatenated_comb_simulation
    sc = [dict(cfg=cfg(), gamma=1.1, alpha=1.15e-2, dispersion=disp(), max_order=3),
          dict(cfg=cfg(30), gamma=1.3, alpha=0.0, dispersion=disp(0.5))]
    cc = dict(spans=sc, omega_center=W0, line_spacing=DW, p_in=P3)
    cc_km = dict(spans=[dict(cfg=cfg(30), gamma=1.1, alpha=0.0, dispersion=disp(1e3)),
                        dict(cfg=cfg(), gamma=1.2, alpha=2e-2, dispersion=disp(2e3), max_order=2)],
                 omega_center=W0, line_spacing=DW, p_in=P5, phase_in=[0.1, 0.2, -0.3, 0.0, 1.0],
                 transfers=[sim.comb_mid_stage([0.0, -1.0, -1.0, 0.0, 3.0], 0.5)], length_unit="km")
    f = sim.run_concatenated_comb_simulation
    valid("cat_comb/m3", f, cc)
    valid("cat_comb/one_span", f, dict(cc, spans=sc[1:]))
    valid("cat_comb/km5_dark", f, cc_km)
    valid("cat_comb/km_to_m", f, dict(cc_km, return_length_unit="m"))
    valid("cat_comb/bad_span0", f, cc, (0, 7))
    valid("cat_comb/bad_span1", f, cc_km, (0, 31))
    valid("cat_comb/bad_unchecked", f, dict(cc, spans=[dict(s, cfg=cfg(20, check_nan=False)) for s in sc]), (0, 7))
    failing("cat_comb", f, cc, [("empty", dict(spans=[])), ("unit", dict(length_unit="mm"))] + comb_rules("p_in")
            + span_rules(sc)[:4] + [("span_disp_none", dict(spans=[sc[0], dict(sc[1], dispersion=None)])),
                                    ("span_no_disp", dict(spans=[_drop(sc[0], "dispersion"), sc[1]]))]
            + span_rules(sc)[4:] + line_rules[:4] + [("span_order_type", dict(spans=[dict(sc[0], max_order=3.0), sc[1]])),
                                                     ("span_order", dict(spans=[sc[0], dict(sc[1], max_order=1)])), line_rules[6],
                                                     ("kappa_inf", dict(spans=[sc[0], dict(sc[1], dispersion=disp(beta2=1e300))]))]
            + end_rules(sc, 3),
            extra_pairs=[("empty", "unit"), ("ph_nan", "unknown"), ("span_disp_none", "wc_neg")])

    # -- scan_wdm_gain
    wdm = dict(cfg=cfg(), lambda_p1_m=L1, lambda_p2_m=L2, Omega=OM3, p_pump=[0.3, 0.2],
               p_signal=[[1e-4, 2e-4, 3e-4], [2e-4, 2e-4, 1e-4], [1e-4, 1e-5, 3e-4], [5e-4, 2e-4, 3e-4]], gamma=1.1, alpha=1.15e-2,
               dispersion=disp())
    wdm1 = dict(wdm, Omega=OM1, p_signal=[1e-4])
    f = scan.scan_wdm_gain
    valid("wdm/k3", f, wdm)
    valid("wdm/k1_one_point", f, wdm1)
    valid("wdm/k3_km_linear_end", f, dict(wdm, cfg=cfg(30), dispersion=disp(1e3), length_unit="km", gain_unit="linear",
                                           gain_mode="end", p_idler=[1e-6, 0.0, 2e-6], phase_in=np.linspace(-1.0, 1.0, 8),
                                           even_orders=(2,)))
    valid("wdm/k3_idler_per_point", f, dict(wdm, p_idler=np.full((4, 3), 1e-6), gain_unit=" DB "))
    valid("wdm/k3_device1", f, dict(wdm, device=1, p_idler=1e-6))
    valid("wdm/k3_devices0", f, dict(wdm, devices=[0]))
    valid("wdm/k3_devices01", f, dict(wdm, devices=[0, 1], device=3))
    valid("wdm/k3_bad", f, wdm, BAD)
    wdm_plan = [
        ("omega_2d", dict(Omega=[OM3])),
        ("omega_many", dict(Omega=[1e12] * 17)),
        ("omega_nan", dict(Omega=[1e12, float("nan"), 2e12])),
        ("pump_shape", dict(p_pump=[0.3])),
        ("pump_neg", dict(p_pump=[0.3, -0.2])),
    ]
    wdm_tail = [
        ("disp_none", dict(dispersion=None)),
        ("lambda", dict(lambda_p1_m=-L1)),
        ("omega_big", dict(Omega=[OM3[0], 3.0 * W0, OM3[2]])),
        ("cfg", dict(cfg=P.config.custom_simulation_config(z_max=2.0, dz=0.1, integrator="rk2"))),
        ("disp_type", dict(dispersion=1)),
    ]
    failing("wdm", f, wdm, [("mode", dict(gain_mode="mean")), ("gunit", dict(gain_unit="neper"))] + wdm_plan + [
        ("sig_shape", dict(p_signal=[1e-4, 2e-4])),
        ("sig_3d", dict(p_signal=np.full((2, 2, 3), 1e-4))),
        ("sig_zero", dict(p_signal=[1e-4, 0.0, 1e-4])),
        ("idler_shape", dict(p_idler=[1e-6, 1e-6])),
        ("idler_neg", dict(p_idler=-1e-6)),
        ("ph_shape", dict(phase_in=[0.0] * 4)),
        ("ph_nan", dict(phase_in=[float("nan")] * 8)),
    ] + wdm_tail + [("unit", dict(length_unit="mile")), ("even", dict(even_orders=(3,))), ("multiple_points", dict(gamma=[1.0, 2.0]))],
        extra_pairs=[("mode", "omega_2d"), ("pump_neg", "sig_zero"), ("idler_neg", "disp_none")])

    # -- scan_single_pump_gain
    lam = [1540e-9, float("nan"), 1548e-9, -1.0, 700e-9, 1561e-9]       # an invalid wavelength twice; 700 nm: idler <= 0
    spg = dict(cfg=cfg(), lambda_pump_m=LAM0, lambda_signal_m=lam, p_pump=0.4, p_signal=1e-4, gamma=1.1, alpha=1.15e-2,
               dispersion=disp())
    f = scan.scan_single_pump_gain
    valid("sp_gain/m", f, spg)
    valid("sp_gain/km_linear_end_f32", f, dict(spg, cfg=cfg(30), dispersion=disp(1e3), length_unit="km", gain_unit="linear",
                                                gain_mode="end", p_idler=1e-6, phase_in=[0.3, 0.0, -0.3], max_order=3,
                                                dtype=np.float32, lambda_signal_m=lam[:5]))
    valid("sp_gain/device1", f, dict(spg, device=1))
    valid("sp_gain/devices0", f, dict(spg, devices=[0], lambda_signal_m=np.array(lam[:3])))
    valid("sp_gain/devices01_f32", f, dict(spg, devices=[0, 1], dtype=np.float32))
    valid("sp_gain/bad", f, spg, BAD)
    valid("sp_gain/dbeta_not_finite", f, dict(spg, dispersion=disp(beta2=1e300)))
    failing("sp_gain", f, spg, [
        ("mode", dict(gain_mode="mean")),
        ("gunit", dict(gain_unit="neper")),
        ("lam_2d", dict(lambda_signal_m=[lam])),
        ("lam_empty", dict(lambda_signal_m=[])),
        ("p_nan", dict(p_pump=float("nan"))),
        ("p_neg", dict(p_idler=-1e-6)),
        ("seed", dict(p_signal=0.0)),
        ("ph_shape", dict(phase_in=[0.0, 0.0])),
        ("ph_nan", dict(phase_in=[0.0, float("nan"), 0.0])),
        ("disp_none", dict(dispersion=None)),
        ("order", dict(max_order=-1)),
        ("lambda_pump", dict(lambda_pump_m=0.0)),
        ("cfg", dict(cfg=cfg(save_every=-1))),
        ("unit", dict(length_unit="mile")),
        ("dtype", dict(dtype=np.float16)),
    ], extra_pairs=[("mode", "lam_2d"), ("seed", "disp_none"), ("order", "cfg")])

    # -- scan_comb_gain
    cg = dict(cfg=cfg(), lambda_center_m=LAM0, line_spacing=DW, p_lines=[P5, P5[::-1], [0.1] * 5, P5], gamma=1.1, alpha=1.15e-2,
              dispersion=disp())
    f = scan.scan_comb_gain
    valid("comb_gain/m5_dark", f, cg)
    valid("comb_gain/m3_one_point", f, dict(cg, p_lines=P3))
    valid("comb_gain/km_linear_end_f32", f, dict(cg, cfg=cfg(30), dispersion=disp(1e3), length_unit="km", gain_unit="linear",
                                                  gain_mode="end", phase_in=[0.3, 0.0, -0.3, 0.1, 0.2], max_order=3,
                                                  dtype=np.float32, p_lines=[P5, P5[::-1], [0.1] * 5, P5, P5]))
    valid("comb_gain/device1", f, dict(cg, device=1))
    valid("comb_gain/devices0", f, dict(cg, devices=[0]))
    valid("comb_gain/devices01_f32", f, dict(cg, devices=[0, 1], dtype=np.float32))
    valid("comb_gain/bad", f, cg, BAD)
    failing("comb_gain", f, cg, [("mode", dict(gain_mode="mean")), ("gunit", dict(gain_unit="neper")), ("dtype", dict(dtype=np.float16))]
            + comb_rules("p_lines")[:5] + [("p_3d", dict(p_lines=np.full((2, 2, 3), 0.1))), ("ph_shape", dict(phase_in=[0.0, 0.0])),
                                           ("ph_nan", dict(phase_in=[0.0, float("nan"), 0.0, 0.0, 0.0])),
                                           ("disp_none", dict(dispersion=None)), ("cfg", dict(cfg=cfg(save_every=0))),
                                           ("lambda", dict(lambda_center_m=float("inf")))] + line_rules[2:],
            extra_pairs=[("dtype", "p_neg"), ("ph_nan", "disp_none"), ("disp_none", "lowest")])

    # -- scan_copier_psa_phase (four waves) and scan_single_pump_copier_psa_phase
    ph5 = np.linspace(0.0, 2.0 * np.pi, 5, endpoint=False)
    for prefix, f, nw, seed, pump in (("psa4", scan.scan_copier_psa_phase, 4, 2, "pumps"),
                                      ("psa_sp", scan.scan_single_pump_copier_psa_phase, 3, 1, "pump")):
        p_in = [0.25, 0.25, 1e-4, 1e-6] if nw == 4 else [0.4, 1e-4, 2e-6]
        ps = dict(psa_cfg=cfg(), psa_delta_beta=-0.3, gamma=1.1, alpha=1.15e-2, p_in=p_in, phase=ph5)
        with_copier = dict(ps, copier_cfg=cfg(30), psa_delta_beta=[-0.3, 0.0, 0.2])
        valid(f"{prefix}/no_copier", f, ps)
        valid(f"{prefix}/default_phase", f, _drop(ps, "phase"))
        valid(f"{prefix}/copier_defaults", f, with_copier)
        valid(f"{prefix}/copier_own_km_linear_end", f, dict(
            with_copier, copier_delta_beta=120.0, copier_gamma=1.4, copier_alpha=0.0, length_unit="km", gain_unit="linear",
            gain_mode="end", phase_in=[0.1] * nw, mid_gain_db=[-1.0] * (nw - 1) + [2.0], mid_phase=[0.0, 0.1, 0.2, 0.3][:nw],
            phase_wave=seed))
        valid(f"{prefix}/copier_gamma_only", f, dict(with_copier, copier_gamma=0.9, phase_wave=np.int64(0)))
        valid(f"{prefix}/copier_alpha_only", f, dict(with_copier, copier_alpha=0.02, phase_wave=nw - 1, psa_delta_beta=[0.1]))
        valid(f"{prefix}/device1", f, dict(with_copier, device=1))
        valid(f"{prefix}/devices0", f, dict(ps, devices=[0]))
        valid(f"{prefix}/devices01", f, dict(with_copier, devices=[0, 1]))
        valid(f"{prefix}/bad", f, with_copier, BAD)
        valid(f"{prefix}/all_bad", f, dict(ps, phase=[0.5]), (0, 7))
        # the mismatch is provided, so no fibre is built from gamma and alpha and none of its rules applies: a gain is a negative alpha
        valid(f"{prefix}/negative_alpha", f, dict(with_copier, alpha=-0.02, copier_gamma=-1.0))
        if nw == 4:
            valid("psa4/f32", f, dict(with_copier, dtype=np.float32))
            valid("psa4/f32_no_copier_devices01", f, dict(ps, dtype=np.float32, devices=[0, 1]))
        else:
            valid("psa_sp/mid_scalars", f, dict(with_copier, mid_gain_db=-1.5, mid_phase=0.25))
        failing(prefix, f, with_copier, [
            ("mode", dict(gain_mode="mean")),
            ("gunit", dict(gain_unit="neper")),
            ("phase_2d", dict(phase=[[0.0, 1.0]])),
            ("phase_empty", dict(phase=[])),
            ("phase_nan", dict(phase=[0.0, float("nan")])),
            ("db_2d", dict(psa_delta_beta=[[0.0, 1.0]])),
            ("db_nan", dict(psa_delta_beta=float("nan"))),
            ("wave_name", dict(phase_wave="signal")),
            ("wave_index", dict(phase_wave=nw)),
            ("p_shape", dict(p_in=p_in[:-1])),
            ("p_neg", dict(p_in=[-0.1] + p_in[1:])),
            ("seed", dict(p_in=p_in[:seed] + [0.0] + p_in[seed + 1:])),
            ("ph0_shape", dict(phase_in=[0.0])),
            ("ph0_nan", dict(phase_in=[float("nan")] * nw)),
            ("psa_cfg", dict(psa_cfg=P.config.custom_simulation_config(z_max=0.0, dz=0.1))),
            ("copier_cfg", dict(copier_cfg=cfg(30, save_every=0))),
            ("unit", dict(length_unit="mm")),
            ("share_save_every", dict(copier_cfg=cfg(30, save_every=5))),
            ("mid_width", dict(mid_gain_db=[0.0] * (nw + 1))),
            ("mid_nan", dict(mid_phase=[float("nan")] * nw)),
            ("multiple", dict(psa_cfg=cfg(25))),
        ], extra_pairs=[("mode", "phase_2d"), ("db_nan", "wave_name"), ("wave_index", "p_neg"), ("ph0_nan", "unit"),
                        ("seed", "mid_width")])
        valid(f"err/{prefix}/share_check_nan", f, dict(with_copier, copier_cfg=cfg(30, check_nan=False)))
        # a bool is an index for the four waves and no index for the three
        valid(("psa4" if nw == 4 else "err/psa_sp") + "/wave_bool", f, dict(with_copier, phase_wave=True))

    # -- scan_wdm_copier_psa_phase
    wl = dict(psa_cfg=cfg(), lambda_p1_m=L1, lambda_p2_m=L2, Omega=OM3, p_pump=[0.3, 0.2], p_signal=[1e-4, 2e-4, 3e-4], gamma=1.1,
              alpha=1.15e-2, dispersion=disp(), phase=ph5)
    wl_c = dict(wl, copier_cfg=cfg(30))
    f = scan.scan_wdm_copier_psa_phase
    valid("psa_wdm/no_copier", f, wl)
    valid("psa_wdm/default_phase_k1", f, _drop(dict(wl, Omega=OM1, p_signal=[1e-4]), "phase"))
    valid("psa_wdm/copier_defaults", f, wl_c)
    valid("psa_wdm/copier_own_km_linear_end", f, dict(
        wl_c, dispersion=disp(1e3), copier_dispersion=disp(2e3), copier_gamma=1.4, copier_alpha=0.0, length_unit="km",
        gain_unit="linear", gain_mode="end", p_idler=[1e-6, 0.0, 2e-6], mid_gain_db=np.linspace(-2.0, 1.0, 8),
        mid_phase=np.linspace(0.0, 0.7, 8), phase_wave="signals", even_orders=(2,)))
    valid("psa_wdm/copier_gamma_only", f, dict(wl_c, copier_gamma=0.9, phase_wave="idlers", mid_gain_db=-1.5))
    valid("psa_wdm/copier_alpha_only", f, dict(wl_c, copier_alpha=0.02, mid_phase=0.25, p_idler=1e-6))
    valid("psa_wdm/copier_dispersion_only", f, dict(wl_c, copier_dispersion=disp(0.5)))
    valid("psa_wdm/device1", f, dict(wl_c, device=1))
    valid("psa_wdm/devices0", f, dict(wl, devices=[0]))
    valid("psa_wdm/devices01", f, dict(wl_c, devices=[0, 1]))
    valid("psa_wdm/bad", f, wl_c, BAD)
    valid("psa_wdm/all_bad", f, dict(wl, phase=[0.5]), (0, 7))
    link_rules = [
        ("psa_cfg", dict(psa_cfg=P.config.custom_simulation_config(z_max=0.0, dz=0.1))),
        ("share_save_every", dict(copier_cfg=cfg(30, save_every=5))),
        ("copier_cfg", dict(copier_cfg=P.config.custom_simulation_config(z_max=3.0, dz=0.1, integrator="euler"))),
        ("unit", dict(length_unit="mm")),
        ("copier_disp_type", dict(copier_dispersion=2.0)),
        ("multiple", dict(psa_cfg=cfg(25))),
    ]
    failing("psa_wdm", f, wl_c, [("mode", dict(gain_mode="mean")), ("gunit", dict(gain_unit="neper")),
                                 ("phase_2d", dict(phase=[[0.0, 1.0]])), ("phase_nan", dict(phase=[0.0, float("nan")]))] + wdm_plan + [
        ("sig_shape", dict(p_signal=[[1e-4, 2e-4, 3e-4]])),
        ("sig_zero", dict(p_signal=[1e-4, 0.0, 1e-4])),
        ("idler_shape", dict(p_idler=np.full((5, 3), 1e-6))),
        ("idler_neg", dict(p_idler=-1e-6)),
        ("wave_name", dict(phase_wave="pump")),
        ("wave_type", dict(phase_wave=0)),
        ("mid_gain_shape", dict(mid_gain_db=[0.0] * 4)),
        ("mid_phase_shape", dict(mid_phase=[[0.0] * 8])),
    ] + wdm_tail[:3] + link_rules + [("even", dict(even_orders=(3,))), ("mid_nan", dict(mid_gain_db=float("inf")))],
        extra_pairs=[("mode", "phase_2d"), ("phase_nan", "omega_2d"), ("idler_neg", "wave_name"), ("mid_phase_shape", "disp_none"),
                     ("omega_big", "share_save_every")])
    valid("err/psa_wdm/share_check_nan", f, dict(wl_c, copier_cfg=cfg(30, check_nan=False)))
    # the two dispersion scans compare the configs before they validate them; the two above after
    valid("err/psa_wdm/copier_save_every_zero", f, dict(wl_c, copier_cfg=cfg(30, save_every=0)))
    valid("err/psa_wdm/negative_alpha", f, dict(wl_c, alpha=-0.02))

    # -- scan_comb_copier_psa_phase
    cl = dict(psa_cfg=cfg(), lambda_center_m=LAM0, line_spacing=DW, p_lines=P5, gamma=1.1, alpha=1.15e-2, dispersion=disp(),
              phase=ph5, phase_lines=(1, 2))
    cl_c = dict(cl, copier_cfg=cfg(30))
    f = scan.scan_comb_copier_psa_phase
    valid("psa_comb/no_copier_dark", f, cl)
    valid("psa_comb/default_phase_m3", f, _drop(dict(cl, p_lines=P3, phase_lines=[1]), "phase"))
    valid("psa_comb/copier_defaults", f, cl_c)
    valid("psa_comb/copier_own_km_linear_end", f, dict(
        cl_c, dispersion=disp(1e3), copier_dispersion=disp(2e3), copier_gamma=1.4, copier_alpha=0.0, length_unit="km",
        gain_unit="linear", gain_mode="end", phase_in=[0.1, 0.2, 0.0, -0.1, 0.3], mid_gain_db=np.linspace(-2.0, 1.0, 5),
        mid_phase=np.linspace(0.0, 0.7, 5), phase_lines=np.array([0, 4]), max_order=3))
    valid("psa_comb/copier_gamma_only", f, dict(cl_c, copier_gamma=0.9, mid_gain_db=-1.5))
    valid("psa_comb/copier_alpha_only", f, dict(cl_c, copier_alpha=0.02, mid_phase=0.25))
    valid("psa_comb/copier_dispersion_only", f, dict(cl_c, copier_dispersion=disp(0.5)))
    valid("psa_comb/device1", f, dict(cl_c, device=1))
    valid("psa_comb/devices0", f, dict(cl, devices=[0]))
    valid("psa_comb/devices01", f, dict(cl_c, devices=[0, 1]))
    valid("psa_comb/bad", f, cl_c, BAD)
    valid("psa_comb/all_bad", f, dict(cl, phase=[0.5]), (0, 7))
    failing("psa_comb", f, cl_c, [("mode", dict(gain_mode="mean")), ("gunit", dict(gain_unit="neper")),
                                  ("phase_2d", dict(phase=[[0.0, 1.0]])), ("phase_nan", dict(phase=[0.0, float("nan")]))]
            + comb_rules("p_lines")[:6] + [
        ("ph_shape", dict(phase_in=[0.0, 0.0])),
        ("ph_nan", dict(phase_in=[0.0, float("nan"), 0.0, 0.0, 0.0])),
        ("lines_none", dict(phase_lines=())),
        ("lines_type", dict(phase_lines=3)),
        ("lines_range", dict(phase_lines=[1, 5])),
        ("lines_twice", dict(phase_lines=[1, 1])),
        ("lines_bool", dict(phase_lines=[True])),
        ("mid_gain_shape", dict(mid_gain_db=[0.0] * 4)),
        ("mid_phase_shape", dict(mid_phase=[[0.0] * 5])),
        ("disp_none", dict(dispersion=None)),
        ("lambda", dict(lambda_center_m=-LAM0)),
    ] + link_rules + line_rules[2:] + [("mid_nan", dict(mid_gain_db=float("inf")))],
        extra_pairs=[("mode", "phase_2d"), ("phase_nan", "p_ndim"), ("ph_nan", "lines_none"), ("mid_phase_shape", "disp_none"),
                     ("lambda", "share_save_every"), ("unit", "lowest")])
    valid("err/psa_comb/share_check_nan", f, dict(cl_c, copier_cfg=cfg(30, check_nan=False)))
    valid("err/psa_comb/copier_save_every_zero", f, dict(cl_c, copier_cfg=cfg(30, save_every=0)))
    valid("err/psa_comb/negative_copier_alpha", f, dict(cl_c, copier_alpha=-0.02))
    valid("err/psa_comb/lines_missing", f, _drop(cl_c, "phase_lines"))
    return out


def run_case(P, case) -> dict:
    """One case over a fresh stand-in -> its record: the sorted native calls and what the driver returned, or what it raised."""
    fn, kw, bad = case
    stand_in = StandIn(bad)
    saved = stand_in.install(P.native)
    try:
        with np.errstate(all="ignore"):
            got = fn(**kw)
    except Exception as e:   # ValueError, TypeError and FloatingPointError by the drivers' rules; anything else is recorded too
        return {"calls": stand_in.sorted_calls(), "raised": [type(e).__name__, str(e)]}
    finally:
        StandIn.restore(P.native, saved)
    return {"calls": stand_in.sorted_calls(), "returned": encode(got)}
