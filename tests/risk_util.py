"""Shared recipes of the ensemble-objective tests (tests/test_ensemble_risk_algebra.py, tests/test_gpu_ensemble_risk.py),
on top of tests/ensemble_util.py: the named ensemble "rank", the reference (member costs and gradients from the oracle,
J̄ and ω from qoc_amd.robust.ensemble_risk, which has the engine's formulas and summation order) and the conditions on
the reference under which the comparison bars hold.

The bars (every measure is W-Lipschitz in the member costs in the max norm):
  member costs against the oracle                              1e-12
  ω against ensemble_risk(the engine's own member costs)       32 ε W   (same formulas; exp / log1p differ by ulps)
  J̄ against ensemble_risk(the oracle's member costs)           1e-12 W
  dJ̄/du against Σ_e ω_e^engine g_e^oracle                      relative 1e-10 per pulse
  ω against ω of the oracle's costs                            W (2 β 1e-12 + 32 ε) for LSE (the softmax's Lipschitz
                                                               constant); 32 ε W for MAX and CVaR, where the conditions
                                                               below make the weights piecewise constant
Conditions asserted on the reference (assert_conditions): member-cost gaps > 1e-9 within every pulse compared, and for
CVaR α W either farther than 1e-6 from every partial sum of the ordered weights or equal to one exactly.
"""
import functools

import numpy as np

import ensemble_util as EU
from ensemble_util import _cavity_detuning

EPS = np.finfo(np.float64).eps
RANK_W = (0.25, 0.25, 0.125, 0.25, 0.125)


@functools.lru_cache(maxsize=None)
def ens_case(name):
    """ensemble_util.ens_case plus "rank": cavity N = 6 (3 blocks of 2), Nt = 16, B = 6, E = 5 with dyadic weights
    (W = 1: α W and the partial sums are exact).  The worst member is 2 for pulses 0, 3, 4, 5 and 3 for pulses 1, 2,
    and the descending orders differ between pulses, so a kernel that ranks by the wrong pulse fails."""
    if name != "rank":
        return EU.ens_case(name)
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=3, Nt=16)
    D = _cavity_detuning(3)
    A0s, As = systems.ensemble_members(p, dA0=[d * D for d in (0.0, 2e-2, -2e-2, 1e-2, -1e-2)],
                                       amp_scales=(1.0, 0.9, 1.1, 1.2, 0.8))
    return p, systems.cavity_controls(6, 16, seed=101, umax=0.3), A0s, As, RANK_W, None


def weights(name):
    w = ens_case(name)[4]
    E = ens_case(name)[2].shape[0]
    return np.full(E, 1.0 / E) if w is None else np.asarray(w, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, order=3, pulses=None):
    """Member costs Jm (B', E) and member gradients gm (B', E, nu, Nt) of the named case's pulses from the oracle (the
    trace cost), read-only and shared."""
    if name != "rank":
        return EU.reference(name, order, False, pulses)[:2]
    prob, u, A0s, As, _, pn = ens_case(name)
    w = weights(name)
    rows = [EU.ensemble_eval(prob, u[b], A0s, As, w, order, pn) for b in (pulses or range(u.shape[0]))]
    out = tuple(np.stack([r[i] for r in rows]) for i in range(2))
    for a in out:
        a.setflags(write=False)
    return out


def assert_conditions(Jm, w, kind, param):
    """The conditions under which the weights are piecewise constant in the costs (module docstring)."""
    for J in np.atleast_2d(Jm):
        gaps = np.abs(J[:, None] - J[None, :])[~np.eye(len(J), dtype=bool)]
        assert gaps.min() > 1e-9, gaps.min()
        if kind == "cvar":
            part = np.cumsum(np.asarray(w)[np.argsort(-J, kind="stable")])
            aW = float(param) * float(np.sum(w))
            d = np.abs(part - aW)
            assert ((d > 1e-6) | (part == aW)).all(), (part, aW)


def omega_bar(w, kind, param):
    """The bar on ω against ω of the oracle's costs."""
    W = float(np.sum(w))
    return W * (2.0 * float(param) * 1e-12 + 32 * EPS) if kind == "lse" else 32 * EPS * W


def assert_risk(J, g, Jm, om, ref, rows, w, kind, param, tag):
    """An engine result (J̄ (B,), dJ̄/du (B, nu, Nt), member costs and ω (B, E)) against the reference's rows: rows[i]
    is the engine's pulse of reference row i."""
    from qoc_amd.robust import ensemble_risk
    Jmr, gmr = ref
    W = float(np.sum(w))
    assert_conditions(Jmr, w, kind, param)
    for i, b in enumerate(rows):
        Jb_r, om_r = ensemble_risk(Jmr[i], w, kind, param)
        _, om_own = ensemble_risk(Jm[b], w, kind, param)
        gref = np.tensordot(om[b], gmr[i], axes=1)
        rel = np.linalg.norm(g[b] - gref) / np.linalg.norm(gref)
        print(tag, b, "max dJm", np.abs(Jm[b] - Jmr[i]).max(), "dJbar", J[b] - Jb_r, "d omega (own costs)",
              np.abs(om[b] - om_own).max(), "d omega (oracle)", np.abs(om[b] - om_r).max(), "rel dJdu", rel)
        assert np.abs(Jm[b] - Jmr[i]).max() <= 1e-12, (tag, b)
        assert np.abs(om[b] - om_own).max() <= 32 * EPS * W, (tag, b, om[b] - om_own)
        assert abs(J[b] - Jb_r) <= 1e-12 * W, (tag, b, J[b] - Jb_r)
        assert rel <= 1e-10, (tag, b, rel)
        assert np.abs(om[b] - om_r).max() <= omega_bar(w, kind, param), (tag, b, om[b] - om_r)
        assert (om[b] >= 0).all() and abs(om[b].sum() - W) <= 32 * EPS * W
