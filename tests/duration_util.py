"""Shared recipes of the gate-duration tests (tests/test_duration_algebra.py, tests/test_gpu_duration.py): the reference
for one seed under a time scale τ and the bars.

Seed b evolves under τ_b (A0 + Σ_j u_jk A_j).  The reference runs oracle/qoc_oracle.grape_eval on the scaled
generators (τ_b A0, τ_b A_j) with the case's penalty / cost, which gives J, dJdu and the cache of states and
co-states; then, with U_k = exp(τ A_k) and [A_k, U_k] = 0,

    dJ/dτ = Σ_k Re<lam[k+1], A_k x[k+1]>,    A_k = A0 + Σ_j u_jk A_j unscaled,

and S = Σ_k |that term| is the natural scale of a sum of Nt cancelling terms.  A reference is computed once per
(problem, pulse, τ, order, cost, penalty) and shared; nobody writes to it.

The bars (every scale comes from the reference, never from the engine's output): the project's fp64 bars
|ΔJ| <= 1e-12 max(1, |J_ref|) and ||ΔdJdu|| / ||dJdu|| <= 1e-10, and |ΔdJ/dτ| <= 1e-10 S, the same gradient bar on
that scale.
"""
import numpy as np

import qoc_oracle as O

EX = "exact"
_cache = {}


def duration_terms(A0, A, u, cache):
    """The Nt terms Re<lam[k+1], A_k x[k+1]> of dJ/dτ from an oracle cache (A0, A unscaled)."""
    Nt = u.shape[1]
    t = np.zeros(Nt)
    for k in range(Nt):
        Ak = np.asarray(A0, dtype=np.complex128) + sum(u[j, k] * np.asarray(A[j]) for j in range(len(A)))
        t[k] = float(np.real(np.vdot(cache.lam[k + 1], Ak @ cache.x[k + 1])))
    return t


def scaled_eval(prob, u, tau, order=3, penalty=None, cost=None):
    """(J, dJdu, dJ/dτ, S, cache) of one pulse u (nu, Nt) at the time scale tau."""
    A0, A = tau * np.asarray(prob.A0), [tau * np.asarray(a) for a in prob.A]
    J, g, cache = O.grape_eval(A0, A, u, prob.x0, prob.x_target, prob.n, order=order, penalty=penalty, cost=cost)
    t = duration_terms(prob.A0, prob.A, np.asarray(u), cache)
    return J, g, float(t.sum()), float(np.abs(t).sum()), cache


def reference(key, prob, u, tau, order=3, zcal=False, penalty=None):
    """scaled_eval without the cache, memoised under (key, τ, order, cost, penalised); key names the problem and pulse."""
    k = (key, float(tau), order, bool(zcal), penalty is not None)
    if k not in _cache:
        cost = O.setup_infidelity_zcalibrated(prob.x_target) if zcal else None
        J, g, d, S, _ = scaled_eval(prob, u, tau, order, penalty, cost)
        g.setflags(write=False)
        _cache[k] = (J, g, d, S)
    return _cache[k]


def assert_seed(J, g, d, ref, tag, zcal_args=None):
    """One seed of an engine result (J, dJdu (nu, Nt), dJ/dτ) against its reference.  zcal_args = (prob, u, tau,
    order): the z-calibrated cost, whose gradients carry the calibration phase of a golden-section search that two
    correct implementations fix only to ~sqrt(eps): dJdu is held by qoc_oracle.zcal_gradient_match and dJ/dτ within
    the one-parameter family d(Δθ) ≈ d(0) + Δθ d'(0), |Δθ| <= qoc_oracle.zcal_dtheta_bound, slack 1e-10 S."""
    Jr, gr, dr, S = ref
    print(tag, "dJ", J - Jr, "ddJdtau / S", (d - dr) / S, "S", S)
    assert abs(J - Jr) <= 1e-12 * max(1.0, abs(Jr)), (tag, J - Jr)
    if zcal_args is None:
        rel = np.linalg.norm(g - gr) / np.linalg.norm(gr)
        print(tag, "rel dJdu", rel)
        assert rel <= 1e-10, (tag, rel)
        assert abs(d - dr) <= 1e-10 * S, (tag, d - dr, S)
        return
    prob, u, tau, order = zcal_args
    A0, A = tau * np.asarray(prob.A0), [tau * np.asarray(a) for a in prob.A]
    res, _ = O.zcal_gradient_match(g, A0, A, u, prob.x0, prob.x_target, order=order)
    print(tag, "zcal residual", res)
    assert res <= 1e-10, (tag, res)

    def dtau(dth):
        cost = O.setup_infidelity_zcalibrated_shifted(prob.x_target, dth)
        return scaled_eval(prob, u, tau, order, None, cost)[2]
    h = 1e-6
    d0, slope = dtau(0.0), (dtau(h) - dtau(-h)) / (2 * h)
    bound = O.zcal_dtheta_bound(prob.x_target, O.propagate(A0, A, u, prob.x0)[-1])
    print(tag, "dJdtau off the family's centre", d - d0, "allowed", abs(slope) * bound + 1e-10 * S)
    assert abs(d - d0) <= abs(slope) * bound + 1e-10 * S, (tag, d - d0, slope, bound, S)
