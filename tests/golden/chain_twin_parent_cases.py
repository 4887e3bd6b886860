"""The cases and the record of tests/golden/chain_twin_parent.json, shared by its generator and tests/test_chain_twin_parent.py:
what ``chain`` and ``direct`` of the three NumPy chain restatements (tests/single_pump_chain_np.py, pairs_chain_np.py,
comb_chain_np.py) return, as the SHA-256 of every array's raw bytes behind its dtype and shape.

Per twin: lossy_case(24) at every width the host tests use, save_every 1 and 50, the gauge on and off, with ``direct`` at both
strides; failing_case() with an identity transfer and closed_form_case() over its pump phases where the twin has one, as
the host tests call them."""
import hashlib

import numpy as np

import comb_chain_np
import pairs_chain_np
import single_pump_chain_np

CHAIN_KEYS = ("rows", "z_out", "a_end", "p_wave_end", "p_wave_max", "first_bad_step")
TWINS = {"single_pump": single_pump_chain_np, "pairs": pairs_chain_np, "comb": comb_chain_np}
WIDTHS = {"single_pump": (None,), "pairs": (1, 2, 3), "comb": (3, 4, 6, 7)}


def digest(x):
    x = np.ascontiguousarray(x)
    return f"{x.dtype.str}{list(x.shape)}:{hashlib.sha256(x.tobytes()).hexdigest()}"


def _single_pump_closed_form():
    c = single_pump_chain_np.closed_form_case()
    F = c["phases"].size
    T = np.ones((F, 3), complex)
    T[:, 0] = np.exp(1j * c["phases"])
    spans = [(L, n, np.full(F, db), c["gamma"], 0.0) for (db, L), n in zip((c["copier"], c["psa"]), c["steps"])]
    return c["a0"], spans, [T]


def _comb_closed_form():
    c = comb_chain_np.closed_form_case()
    T = np.ones((c["phases"].size, 3), complex)
    T[:, 1] = np.exp(1j * c["phases"])
    return c["a0"], [(L, n, c["kappa"], c["gamma"], 0.0) for L, n in zip(c["lengths"], c["steps"])], [T]


def cases():
    """-> {key: (twin module, (a0, spans, transfers), save_every, gauge or None for ``direct``)}."""
    out = {}
    for name, twin in TWINS.items():
        for width in WIDTHS[name]:
            case = twin.lossy_case(24) if width is None else twin.lossy_case(24, width)
            tag = name if width is None else f"{name}-{width}"
            for se in (1, 50):
                out[f"{tag}/lossy/direct/se{se}"] = (twin, case, se, None)
                for gauge in (True, False):
                    out[f"{tag}/lossy/chain/se{se}/{'gauge' if gauge else 'forgot'}"] = (twin, case, se, gauge)
    for name, twin in (("pairs", pairs_chain_np), ("comb", comb_chain_np)):
        a0, spans = twin.failing_case()
        out[f"{name}/failing/chain/se10/gauge"] = (twin, (a0, spans, [np.ones(a0.shape[1])]), 10, True)
    for name, twin, case in (("single_pump", single_pump_chain_np, _single_pump_closed_form()),
                             ("comb", comb_chain_np, _comb_closed_form())):
        out[f"{name}/closed_form/direct/se50"] = (twin, case, 50, None)
        out[f"{name}/closed_form/chain/se50/gauge"] = (twin, case, 50, True)
    return out


def run_case(case):
    twin, (a0, spans, transfers), se, gauge = case
    if gauge is None:
        with np.errstate(all="ignore"):
            return {"direct": digest(twin.direct(a0, spans, transfers, se))}
    r = twin.chain(a0, spans, transfers, se, gauge=gauge)
    return {key: digest(r[key]) for key in CHAIN_KEYS}
