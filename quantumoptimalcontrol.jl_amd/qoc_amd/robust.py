"""Risk measures over a generator ensemble (include/qoc.h qoc_set_ensemble_objective), in numpy.

With member costs J_e of one pulse and the ensemble's weights w_e >= 0, W = Σ_e w_e (added in ascending e), every
objective is a value J̄ and member weights ω_e >= 0 with Σ_e ω_e = W and dJ̄/du = Σ_e ω_e dJ_e/du:

  "mean"          ω_e = w_e, J̄ = Σ_e w_e J_e.
  "max"           e* = argmax J_e over w_e > 0 (the lowest e wins ties); ω_{e*} = W, the others 0; J̄ = W J_{e*}.
  "cvar", α       the members ordered by J descending (ties: ascending e); before_e = Σ w_f over the members ahead of
                  e (added in ascending f); ω_e = min(w_e, max(0, α W - before_e)) / α; J̄ = Σ_e ω_e J_e.  α in (0, 1];
                  α = 1 is the mean, an α no larger than the worst member's share the maximum.
  "lse", β        M = max J_e over w_e > 0, d_e = J_e - M, s = Σ_e (w_e / W) expm1(β d_e),
                  J̄ = W (M + log1p(s) / β), ω_e = w_e exp(β d_e) / (1 + s).  β > 0, finite.  (The plain
                  log Σ exp form loses ε / β to cancellation at small β.)

Sums over the members run in ascending e from 0; a member whose ω_e is exactly 0 is skipped (not multiplied by zero);
if any J_e with w_e > 0 is not finite, every ω_e of the pulse and J̄ are NaN.  Members with w_e = 0 never carry weight
and never enter a maximum.  These are the engine's formulas in the engine's order (k_ens_weights): the device differs
by its fused multiply-adds and by the ulps of its exp / expm1 / log1p.

ensemble_risk is for post-processing GrapeEngine.member_costs() and is the reference of the tests.
"""
from __future__ import annotations

import numpy as np

KINDS = ("mean", "max", "cvar", "lse")


def _check(kind, param):
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
    if kind == "cvar" and not (param is not None and 0.0 < float(param) <= 1.0):
        raise ValueError(f"cvar needs alpha in (0, 1] (got {param!r})")
    if kind == "lse" and not (param is not None and np.isfinite(float(param)) and float(param) > 0.0):
        raise ValueError(f"lse needs a finite beta > 0 (got {param!r})")


def _total(w):
    W = 0.0
    for x in w:
        W += float(x)
    return W


def _one(J, w, kind, param):
    E = J.shape[0]
    W = _total(w)
    pos = w > 0.0
    om = np.zeros(E)
    if not np.isfinite(J[pos]).all():
        return np.nan, np.full(E, np.nan)
    if kind == "mean":
        om[:] = w
    elif kind == "max":
        best = -1
        for e in range(E):
            if pos[e] and (best < 0 or J[e] > J[best]):
                best = e
        om[best] = W
    elif kind == "cvar":
        a = float(param)
        aW = a * W
        for e in range(E):
            before = 0.0
            for f in range(E):
                if J[f] > J[e] or (J[f] == J[e] and f < e):
                    before += w[f]
            om[e] = min(w[e], max(0.0, aW - before)) / a
    else:
        b = float(param)
        M = J[pos].max()
        s = 0.0
        for e in range(E):
            if pos[e]:
                s += (w[e] / W) * np.expm1(b * (J[e] - M))
        for e in range(E):
            if pos[e]:
                om[e] = w[e] * np.exp(b * (J[e] - M)) / (1.0 + s)
        return W * (M + np.log1p(s) / b), om
    Jbar = 0.0
    for e in range(E):
        if om[e] != 0.0:
            Jbar += om[e] * J[e]
    return Jbar, om


def ensemble_risk(Jm, w, kind="mean", param=None):
    """(J̄, ω) of member costs Jm (E,) or (B, E) under weights w (E,): J̄ a float or (B,), ω shaped like Jm."""
    _check(kind, param)
    Jm = np.asarray(Jm, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 1 or Jm.shape[-1] != w.shape[0] or Jm.ndim not in (1, 2):
        raise ValueError(f"Jm {Jm.shape} and w {w.shape} do not match")
    if not (np.isfinite(w).all() and (w >= 0).all() and w.sum() > 0):
        raise ValueError("the weights must be finite, >= 0 and have a positive sum")
    if Jm.ndim == 1:
        Jb, om = _one(Jm, w, kind, param)
        return float(Jb), om
    rows = [_one(J, w, kind, param) for J in Jm]
    return np.array([r[0] for r in rows]), np.stack([r[1] for r in rows])


def active_bound(w, alpha):
    """The most members that can carry weight under CVaR at level alpha, whatever the costs: 1 + the largest k for
    which the k smallest positive weights sum to less than alpha W.  (The worst-case objective: alpha -> 0, 1.)  The
    engine chooses its eval route from this number and the ensemble size alone, never from data."""
    w = np.asarray(w, dtype=np.float64)
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"alpha must be in (0, 1] (got {alpha!r})")
    aW = float(alpha) * _total(w)
    k, acc = 0, 0.0
    for x in sorted(float(v) for v in w if v > 0.0):
        acc += x
        if not acc < aW:
            break
        k += 1
    npos = int((w > 0).sum())
    return min(1 + k, npos)
