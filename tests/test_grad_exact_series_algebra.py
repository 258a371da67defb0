"""The exact gradient on dense generators as a series (csrc/qoc_grad_rr.hpp k_grad_rr_xq / _xp), on the CPU: the
recurrence the kernels run, restated in numpy (tests/gradx_util.py), against the oracle's exact gradient (one 2N x 2N
block exponential per slice and control), and the ABI of its counters.

Bar: 1e-13 relative per seed.  The series' truncation tail is below 2^-53 by the term-count rule and its rounding error
grows like e^ρ ε with ρ the spectral half-width of the shifted slice generator (below the 1-norm that sets the term
count; the controls x 22 reach the largest: 1e-13 e^ρ ε would allow ρ = 6.8, 3.3e-15 observed); the oracle's Padé block
exponential is good to about 1e-15 itself.
"""
import ctypes
import math

import numpy as np
import pytest

import qoc_oracle as O
from gradx_util import exact_terms, gue_problem, rho_of, series_grad, series_unit, shifts


def _cases():
    from qoc_amd import systems
    out = []
    for nc, Nt, scale in ((4, 7, 1.0), (9, 13, 1.0), (20, 9, 1.0), (20, 9, 22.0)):
        p = systems.cavity_dense_problem(nc, Nt)
        out.append((f"cavity_dense{nc}x{scale:g}", p, systems.cavity_controls(1, Nt, seed=nc)[0] * scale))
    p, u = gue_problem(33, 2, 2, 5, seed=7, nrm0=3.6, nrmj=0.4)
    out.append(("gue33", p, u[0]))
    return out


@pytest.mark.parametrize("idx", range(5))
def test_series_matches_the_oracles_exact_gradient(idx):
    name, prob, u = _cases()[idx]
    _, g0, cache = O.grape_eval(prob.A0, prob.A, u, prob.x0, prob.x_target, prob.n, order="exact")
    _, _, nrm = shifts(prob)
    g, ns = series_grad(prob, u, cache, nrm)  # the 1-norm bound
    rel = np.linalg.norm(g - g0) / np.linalg.norm(g0)
    print(name, "rho", rho_of(nrm, u).min(), rho_of(nrm, u).max(), "n", min(ns), max(ns), "rel", rel)
    assert rel <= 1e-13, (name, rel)
    # the truncation matters on these systems: order 3 is far outside the bar
    g3 = O.grape_eval(prob.A0, prob.A, u, prob.x0, prob.x_target, prob.n, order=3)[1]
    assert np.linalg.norm(g3 - g0) / np.linalg.norm(g0) > 1e-6


def test_term_rule():
    """The rule's values quoted in csrc/qoc_common.hpp and the bound it promises."""
    assert exact_terms(0.063) == 9 and exact_terms(0.17) == 11 and exact_terms(1.25) == 20
    assert exact_terms(0.0) == 1 and exact_terms(100.0) == 64
    def bound(rho, n):  # ρ^n / n! / (1 - ρ / (n+1))
        return rho ** n / math.factorial(n) / (1.0 - rho / (n + 1)) if rho < n + 1 else math.inf
    for rho in (0.01, 0.3, 2.0, 8.0):
        n = exact_terms(rho)
        assert bound(rho, n) <= 2.0 ** -53 < bound(rho, n - 1), (rho, n)


def test_zeroed_coefficients_equal_the_short_series_bitwise():
    """A lane whose c_b are zero beyond its own n_k, looping as long as its tile's largest count, gives bitwise what n_k
    terms alone give: its R(b) are exactly zero for b >= n_k."""
    from qoc_amd import systems
    prob = systems.cavity_dense_problem(9, 3)
    rng = np.random.default_rng(3)
    N, m = prob.N, prob.m
    u = np.array([0.03, -0.04])
    Ak = prob.A0 + u[0] * prob.A[0] + u[1] * prob.A[1]
    mu, _, _ = shifts(prob)
    mu_k = mu[0] + u @ mu[1:]
    lam = rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))
    x = rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))
    for n in (1, 5, 12):
        short = series_unit(Ak, prob.A, mu_k, lam, x, n)
        for n_loop in (n + 1, n + 7, 48):
            assert np.array_equal(series_unit(Ak, prob.A, mu_k, lam, x, n, n_loop), short), (n, n_loop)


def test_stats_abi_rejects_null(built_lib):
    """qoc_exact_series_stats: QOC_ERR_ARG for a NULL context or buffer, before anything touches a device."""
    buf = (ctypes.c_longlong * 4)(7, 7, 7, 7)
    assert built_lib.qoc_exact_series_stats(None, buf, 0) == -1
    assert built_lib.qoc_exact_series_stats(None, None, 1) == -1
    assert list(buf) == [7, 7, 7, 7]
    assert b"null" in built_lib.qoc_last_error(None)
