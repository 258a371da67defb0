"""CPU: the algebra of the gate-duration derivative (include/qoc.h qoc_set_time_scale), on the oracle alone.

With U_k = exp(τ A_k) and [A_k, U_k] = 0 the derivative of J with respect to the time scale needs no new propagation:
dJ/dτ = Σ_k Re<λ_{k+1}, A_k x_{k+1}> with the full co-state (the penalty's sources included).  The kernel accumulates
it per block as Re tr(A_k[β] G_{k+1}[β]), G = Σ_c x λ^H, or as Re tr(A_k K_k U_k) with G_k before its own source.
"""
import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import block_problem, case
from duration_util import duration_terms, scaled_eval

H = 1e-5


def _J(prob, u, tau, penalty, cost):
    A0, A = tau * np.asarray(prob.A0), [tau * np.asarray(a) for a in prob.A]
    x = O.propagate(A0, A, u, prob.x0)
    Jf = (cost if cost is not None else O.setup_infidelity(prob.x_target, prob.n))[0]
    L = O.setup_state_penalty(*penalty)[0] if penalty is not None else None
    return Jf(x[-1]) + (sum(L(xk) for xk in x) if L is not None else 0.0)


@pytest.mark.parametrize("tau", [0.8, 1.0, 1.37])
@pytest.mark.parametrize("name,pen,zcal", [("cavity20", False, False), ("cavity20", True, False), ("zz", False, False),
                                            ("zz", True, False), ("zz", False, True)])
def test_formula_against_finite_differences(name, pen, zcal, tau):
    """The formula against the four-point central difference of the oracle's J(τ), h = 1e-5, seed 0.  Bar 1e-6 S
    (S = Σ_k |term|): observed <= 3.2e-8 S; the margin covers the finite difference's own ε J / h noise at J ≈ 10 (the
    penalised cavity)."""
    prob, u, pn = case(name)
    penalty = pn if pen else None
    cost = O.setup_infidelity_zcalibrated(prob.x_target) if zcal else None
    _, _, d, S, _ = scaled_eval(prob, u[0], tau, 3, penalty, cost)
    Jp2, Jp1, Jm1, Jm2 = (_J(prob, u[0], tau + q * H, penalty, cost) for q in (2, 1, -1, -2))
    fd = (-Jp2 + 8 * Jp1 - 8 * Jm1 + Jm2) / (12 * H)
    print(name, pen, zcal, tau, "formula", d, "fd", fd, "diff / S", (d - fd) / S)
    assert abs(d - fd) <= 1e-6 * S


@pytest.mark.parametrize("shape,seed", [((3, 3, 2, 2), 11), ((2, 4, 1, 2), 12)])
def test_block_form(shape, seed):
    """Permuted blocks, the last one a row short (a padding row in the kernel): the per-block traces
    Σ_β Re tr(A_k[β] G_{k+1}[β]) sum to the full-space term, to 1e-13 S, and so does Re tr(A_k K_k U_k), K_k = Σ_c x_k
    λ_{k+1}^H, where K_k U_k is G_k before its own penalty source."""
    NB, nblk, nu, m = shape
    prob, u, blocks = block_problem(NB, nblk, nu, m, 23, seed)
    penalty = ((blocks[0][0], blocks[-1][0]), (0,), 0.37)
    tau = 1.3
    for b in range(2):
        _, _, d, S, cache = scaled_eval(prob, u[b], tau, 3, penalty)
        full = duration_terms(prob.A0, prob.A, u[b], cache)
        assert abs(full.sum() - d) <= 1e-15 * S
        blk = np.zeros(prob.Nt)
        kuk = np.zeros(prob.Nt)
        for k in range(prob.Nt):
            Ak = np.asarray(prob.A0) + sum(u[b][j, k] * np.asarray(prob.A[j]) for j in range(nu))
            G = cache.x[k + 1] @ cache.lam[k + 1].conj().T
            K = cache.x[k] @ cache.lam[k + 1].conj().T
            Gk = K @ cache.Uk[k]  # x_k (U_k^H λ_{k+1})^H: λ_k without its source
            for rows in blocks:
                ix = np.ix_(rows, rows)
                blk[k] += np.trace(Ak[ix] @ G[ix]).real
                kuk[k] += np.trace(Ak[ix] @ Gk[ix]).real
        print(shape, b, "S", S, "block form", np.abs(blk - full).max() / S, "K U form", np.abs(kuk - full).max() / S)
        assert abs(blk.sum() - d) <= 1e-13 * S and np.abs(blk - full).max() <= 1e-13 * S
        assert abs(kuk.sum() - d) <= 1e-13 * S and np.abs(kuk - full).max() <= 1e-13 * S


class _StubEngine:
    """J_b = τ_b Σ_{s,j} w_sj c_bsj² + sin τ_b, with distinct weights so that a misplaced coefficient shows."""

    def __init__(self, B, nu):
        self.B, self.nu, self.ns, self.device = B, nu, 0, 0
        self.tau = None

    def set_spline_basis(self, Bs):
        self.ns = np.asarray(Bs).shape[1]
        self.w = 1.0 + np.arange(self.ns * self.nu, dtype=np.float64).reshape(self.ns, self.nu) / 7.0

    def set_time_scale(self, tau):
        self.tau = np.array(tau, dtype=np.float64)

    def eval_spline(self, c, order=3):
        c = np.asarray(c).reshape(self.B, self.ns, self.nu)
        self.q = (self.w * c * c).sum((1, 2))
        return self.tau * self.q + np.sin(self.tau), 2 * self.tau[:, None, None] * self.w * c

    def time_scale_grad(self):
        return self.q + np.cos(self.tau)


def test_spline_grape_duration_on_a_stub_engine():
    """SplineGrapeDuration.fg: z = [c (index s + ns j), τ] per seed, f = J + κ τ, grad = [dJ/dc in c's layout,
    dJ/dτ + κ]; the gradient is also held against central differences of f itself."""
    from qoc_amd.optimize import SplineGrapeDuration
    B, ns, nu, kappa = 3, 4, 2, 0.05
    eng = _StubEngine(B, nu)
    obj = SplineGrapeDuration(eng, np.zeros((9, ns)), order=3, time_weight=kappa)
    assert (obj.nc, obj.n) == (ns * nu, ns * nu + 1)
    rng = np.random.default_rng(3)
    z = rng.uniform(-1, 1, size=(B, ns * nu + 1))
    z[:, -1] = (0.7, 1.0, 1.6)
    f, g = (a.numpy() for a in obj.fg(z))
    assert np.array_equal(eng.tau, z[:, -1])
    c = z[:, :-1].reshape(B, nu, ns).transpose(0, 2, 1)  # (B, ns, nu): c[b, s, j] = z[b, s + ns j]
    J = z[:, -1] * (eng.w * c * c).sum((1, 2)) + np.sin(z[:, -1])
    np.testing.assert_allclose(f, J + kappa * z[:, -1], rtol=0, atol=1e-14)
    for s in range(ns):
        for j in range(nu):
            np.testing.assert_allclose(g[:, s + ns * j], 2 * z[:, -1] * eng.w[s, j] * c[:, s, j], rtol=0, atol=1e-14)
    np.testing.assert_allclose(g[:, -1], (eng.w * c * c).sum((1, 2)) + np.cos(z[:, -1]) + kappa, rtol=0, atol=1e-14)
    h = 1e-6
    for i in range(ns * nu + 1):
        zp, zm = z.copy(), z.copy()
        zp[:, i] += h
        zm[:, i] -= h
        fd = (obj.fg(zp)[0].numpy() - obj.fg(zm)[0].numpy()) / (2 * h)
        assert np.abs(fd - g[:, i]).max() <= 1e-8
