"""The algebra of the exact gradient on the interpolating block propagators (csrc/qoc_blkp.hpp k_blkp_grad_exact,
csrc/qoc_run_blkp.hip blkp_interp_coeffs), emulated in NumPy without a GPU:
  U(u) = e^{μ(u)} Σ_{i<=D} T_i(ξ) M_i,  ξ = xa u + xb,  μ(u) = μ_0 + u μ_1  (the shifted generators Ã_j = A_j - μ_j I)
  dU/du = e^{μ(u)} Σ_{i<=E} T_i(ξ) N_i,  N_i = μ_1 M_i + xa M'_i,  M'_{i-1} = M'_{i+1} + 2 i M_i,  M'_0 halved
The coefficients as the host forms them (40 Chebyshev points, long double, the series cut where its tail is <= 2^-56,
then differentiated), the sums as the kernel runs them (the Chebyshev recurrence in fp64, the full layout and the packed
upper triangle with both orderings on its off-diagonal entries), against the oracle's block-exponential Fréchet
derivative O.expm_frechet_block at 1e-11 of its largest entry.
"""
import numpy as np
import pytest

import qoc_oracle as O

LD, CLD = np.longdouble, np.clongdouble
NI = 40
TOL = 2.0 ** -56


def _ld_expm(X):
    """exp(X) in long double: scaling to ||X||_1 <= 1/2, Taylor degree 30, squarings (ld_expm of the host code)."""
    n = X.shape[0]
    n1, s = float(np.abs(X).sum(axis=0).max()), 0
    while n1 > 0.5:
        n1 *= 0.5
        s += 1
    Y = X * LD(2.0) ** -s
    E = np.eye(n, dtype=CLD)
    T = np.eye(n, dtype=CLD)
    for k in range(1, 31):
        T = (T @ Y) / LD(k)
        E = E + T
    for _ in range(s):
        E = E @ E
    return E


def _coeffs(A0, A1, mu0, mu1, lo, hi):
    """(M_0..M_D, N_0..N_E) in fp64 from the long-double transform, xa, xb."""
    n = A0.shape[0]
    At0 = (A0 - mu0 * np.eye(n)).astype(CLD)
    At1 = (A1 - mu1 * np.eye(n)).astype(CLD)
    lo, hi = LD(lo), LD(hi)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    pi = np.arccos(LD(-1))
    M = np.zeros((NI, n, n), dtype=CLD)
    for k in range(NI):
        th = pi * (k + LD(0.5)) / NI
        F = _ld_expm(At0 + (mid + half * np.cos(th)) * At1)
        for i in range(NI):
            M[i] += np.cos(i * th) * (2 if i else 1) / NI * F
    mx = np.maximum(np.abs(M.real), np.abs(M.imag)).max(axis=(1, 2))
    assert mx[NI - 1] <= TOL and mx[NI - 2] <= TOL, "the series has not converged"
    D = NI - 1
    while D > 0 and mx[D] <= TOL:
        D -= 1
    Mp = np.zeros((D + 3, n, n), dtype=CLD)
    for i in range(D, 0, -1):
        Mp[i - 1] = Mp[i + 1] + 2 * i * M[i]
    Mp[0] /= 2  # the halved M'_0
    Nc = CLD(mu1) * M[:D + 1] + Mp[:D + 1] / half
    mxn = np.maximum(np.abs(Nc.real), np.abs(Nc.imag)).max(axis=(1, 2))
    E = D
    while E > 0 and mxn[E] <= TOL:
        E -= 1
    xa, xb = float(1 / half), float(-(hi + lo) / (hi - lo))
    return M[:D + 1].astype(np.complex128), Nc[:E + 1].astype(np.complex128), xa, xb


def _cheb_sum(C, xi):
    """Σ_i T_i(ξ) C_i by the kernel's recurrence: T_1 = ξ, T_{i+1} = 2 ξ T_i - T_{i-1}."""
    acc = np.zeros_like(C[0])
    tm = tc = 1.0
    for i in range(len(C)):
        acc = acc + tc * C[i]
        tn = xi if i == 0 else 2.0 * xi * tc - tm
        tm, tc = tc, tn
    return acc


def _contract_full(dU, lam, x):
    """Σ_{r,c,col} conj(λ[r, col]) dU[r][c] x[c, col], entry by entry"""
    return sum(np.conj(lam[r, col]) * dU[r, c] * x[c, col]
               for r in range(dU.shape[0]) for c in range(dU.shape[1]) for col in range(x.shape[1]))


def _contract_triangle(dU, lam, x):
    """the same from the packed upper triangle: an off-diagonal entry weighs both orderings"""
    s = 0.0
    for a in range(dU.shape[0]):
        for b in range(a, dU.shape[0]):
            for col in range(x.shape[1]):
                w = np.conj(lam[a, col]) * x[b, col]
                if b != a:
                    w += np.conj(lam[b, col]) * x[a, col]
                s += w * dU[a, b]
    return s


def _check(A0, A1, mu0, mu1, us, lo, hi, symmetric, rng):
    M, Nc, xa, xb = _coeffs(A0, A1, mu0, mu1, lo, hi)
    print("degrees", len(M) - 1, len(Nc) - 1)
    n = A0.shape[0]
    worst = 0.0
    for u in us:
        xi = xa * u + xb
        ph = np.exp(mu0 + u * mu1)
        U = ph * _cheb_sum(M, xi)
        dU = ph * _cheb_sum(Nc, xi)
        Ur, Lr = O.expm_frechet_block(A0 + u * A1, A1)
        sc = np.abs(Lr).max()
        worst = max(worst, np.abs(dU - Lr).max() / sc)
        assert np.abs(U - Ur).max() <= 1e-13, u
        assert np.abs(dU - Lr).max() <= 1e-11 * sc, (u, np.abs(dU - Lr).max() / sc)
        lam = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        x = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        ref = O.compute_u_sensitivity(x, lam, Lr)
        full = _contract_full(dU, lam, x)
        assert abs(full.real - ref) <= 1e-11 * sc * n * n, (u, full.real, ref)
        if symmetric:
            assert np.abs(dU - dU.T).max() <= 1e-14 * sc
            tri = _contract_triangle(dU, lam, x)
            assert abs(tri - full) <= 1e-12 * abs(full) + 1e-13 * sc, (u, tri, full)
    print("max |dU - L| / max |L|", worst)


def _shift(A):
    """a shift as the engine chooses it: the diagonal's midrange"""
    d = A.diagonal()
    return 0.5 * (d.real.min() + d.real.max()) + 0.5j * (d.imag.min() + d.imag.max())


def test_tunable_bus_block_nt48():
    """The live 14-row parity block of the tunable bus at Nt = 48 (symmetric generators, ||A_k||_1 ~ 30, a purely
    imaginary μ_1): U and dU/du at the batch's controls, on the 5 % widened range; the triangle against the full sum."""
    from qoc_amd import systems
    Nt = 48
    prob = systems.tunable_bus_problem(Nt=Nt, tgate=350.0 * Nt / 2000)
    u = systems.tunable_bus_controls(3, Nt, seed=81)[0, 0]
    rows = np.arange(0, 27, 2)
    A0, A1 = prob.A0[np.ix_(rows, rows)], prob.A[0][np.ix_(rows, rows)]
    assert np.array_equal(A0, A0.T) and np.array_equal(A1, A1.T)
    mu1 = _shift(A1)
    assert mu1.real == 0.0 and mu1.imag != 0.0
    w = u.max() - u.min()
    _check(A0, A1, _shift(A0), mu1, np.concatenate([u[:12], [u.min(), u.max()]]), u.min() - 0.05 * w, u.max() + 0.05 * w,
           True, np.random.default_rng(2))


def test_random_non_symmetric_block():
    """A random 9-row block that is neither symmetric nor skew-Hermitian, with a complex μ_1 (both parts nonzero): the
    μ_1 M_i term and the halved M'_0 carry weight (dropping either fails by orders of magnitude)."""
    rng = np.random.default_rng(11)
    n = 9
    A0 = 0.3 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    A1 = 0.2 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) + (0.4 - 0.7j) * np.eye(n)
    mu1 = _shift(A1)
    assert mu1.real != 0.0 and mu1.imag != 0.0
    us = rng.uniform(-1.0, 1.0, size=10)
    _check(A0, A1, _shift(A0), mu1, np.concatenate([us, [-1.0, 1.0]]), -1.1, 1.1, False, rng)


@pytest.mark.parametrize("drop", ["mu1", "halve"])
def test_the_terms_matter(drop):
    """Without the μ_1 M_i term, or with M'_0 not halved, the random block's dU/du misses the Fréchet derivative by far
    more than the bar: the checks above can tell."""
    rng = np.random.default_rng(11)
    n = 9
    A0 = 0.3 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    A1 = 0.2 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) + (0.4 - 0.7j) * np.eye(n)
    mu0, mu1 = _shift(A0), _shift(A1)
    M, Nc, xa, xb = _coeffs(A0, A1, mu0, mu1, -1.1, 1.1)
    u = 0.37
    xi = xa * u + xb
    Lr = O.expm_frechet_block(A0 + u * A1, A1)[1]
    if drop == "mu1":
        bad = Nc - mu1 * M[:len(Nc)]
    else:
        Mp0 = Nc[0] - mu1 * M[0]  # xa M'_0, halved
        bad = Nc.copy()
        bad[0] += Mp0
    dU = np.exp(mu0 + u * mu1) * _cheb_sum(bad, xi)
    assert np.abs(dU - Lr).max() > 1e-3 * np.abs(Lr).max()
