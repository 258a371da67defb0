"""Shared recipes of the dense exact-series gradient's tests (tests/test_grad_exact_series_algebra.py,
tests/test_gpu_grad_exact_series.py): the term-count rule and the per-generator shifts and bounds restated in
Python, and the series itself in numpy, in the order the kernels run it (csrc/qoc_grad_rr.hpp k_grad_rr_x*):

    λ' = conj(e^{μ_k}) λ_{k+1},  R(n) = 0,  R(b) = c_b λ' + Ã_k^H R(b+1),  c_b = 1 / (b+1)!
    dJdu[j, k] = Re Σ_{b < n} <R(b), A_j q_b>,  q_0 = x_k,  q_{b+1} = Ã_k q_b,  Ã_k = A_k - μ_k I.
"""
import math

import numpy as np

NEX_MAX = 64    # blkseg_exact_terms' own cap (csrc/qoc_common.hpp)
GRADX_NMAX = 48  # above it the engine runs the block exponential (csrc/qoc_grad_rr.hpp)


def exact_terms(rho):
    """blkseg_exact_terms: the smallest n with ρ^n / n! / (1 - ρ / (n+1)) <= 2^-53, capped at 64."""
    tol = 2.0 ** -53
    term, n = 1.0, 0
    while n < NEX_MAX:
        if n >= 1 and rho < n + 1 and term <= tol * (1.0 - rho / (n + 1)):
            break
        n += 1
        term *= rho / n
    return n


def shifts(prob):
    """Per generator j = 0..nu of skew-Hermitian generators A_j = -i H_j: the shift μ_j = -i c_j (c_j the centre of
    H_j's spectrum), the spectral half-width rad_j and the 1-norm nrm_j of the shifted generator."""
    mu, rad, nrm = [], [], []
    for A in [prob.A0] + list(prob.A):
        A = np.asarray(A, dtype=np.complex128)
        assert np.abs(A + A.conj().T).max() <= 1e-13 * max(np.abs(A).max(), 1e-300)
        ev = np.linalg.eigvalsh(1j * A)
        cen = 0.5 * (ev[0] + ev[-1])
        mu.append(-1j * cen)
        rad.append(0.5 * (ev[-1] - ev[0]))
        nrm.append(np.abs(A - (-1j * cen) * np.eye(A.shape[0])).sum(axis=0).max())
    return np.array(mu), np.array(rad), np.array(nrm)


def rho_of(bound, u):
    """ρ_k = bound_0 + Σ_j |u_jk| bound_j for u of shape (nu, Nt)."""
    return bound[0] + np.abs(np.asarray(u)).T @ bound[1:]


def series_unit(Ak, Aj, mu_k, lam, x, n, n_loop=None):
    """dJdu of one (seed, slice) for every control: n terms; the loop runs n_loop >= n times with c_b = 0 for b >= n,
    as a lane does beside a tile mate that needs more terms."""
    n_loop = n if n_loop is None else n_loop
    N = Ak.shape[0]
    At = Ak - mu_k * np.eye(N)
    AtH = At.conj().T
    lp = np.conj(np.exp(mu_k)) * lam
    c = [1.0 / math.factorial(b + 1) for b in range(n_loop)]
    R = [None] * n_loop
    r = np.zeros_like(lp)
    for b in range(n_loop - 1, -1, -1):
        r = (c[b] if b < n else 0.0) * lp + AtH @ r
        R[b] = r
    q = np.array(x, dtype=np.complex128)
    out = np.zeros(len(Aj))
    for b in range(n_loop):
        for j, A in enumerate(Aj):
            out[j] += float(np.real(np.sum(np.conj(R[b]) * (A @ q))))
        q = At @ q
    return out


def series_grad(prob, u, cache, bound):
    """dJdu (nu, Nt) of one seed from the oracle's states and co-states (cache of O.grape_eval) by the series, with n_k
    from the rule at ρ_k = rho_of(bound, u); also returns the n_k."""
    mu, _, _ = shifts(prob)
    u = np.asarray(u, dtype=np.float64)
    rho = rho_of(bound, u)
    g = np.zeros_like(u)
    ns = []
    for k in range(u.shape[1]):
        Ak = np.asarray(prob.A0, dtype=np.complex128) + sum(u[j, k] * np.asarray(prob.A[j]) for j in range(len(prob.A)))
        mu_k = mu[0] + u[:, k] @ mu[1:]
        n = exact_terms(rho[k])
        ns.append(n)
        g[:, k] = series_unit(Ak, prob.A, mu_k, cache.lam[k + 1], cache.x[k], n)
    return g, ns


def gue_problem(N, m, nu, Nt, seed, nrm0=2.0, nrmj=1.0):
    """Random skew-Hermitian generators -i H (H GUE) scaled so that the shifted generators' 1-norms are nrm0 (drift) and
    nrmj (controls), random orthonormal x0 and target of m columns.  With |u| <= 1 the slices' 1-norm bounds ρ_k lie in
    [nrm0, nrm0 + nu nrmj]; the spectral half-widths are about 3.5 times smaller at these sizes."""
    from qoc_amd import systems
    rng = np.random.default_rng(seed)

    def gen(r):
        H = systems._gue(rng, N)
        ev = np.linalg.eigvalsh(H)
        return -1j * H * (r / np.abs(H - 0.5 * (ev[0] + ev[-1]) * np.eye(N)).sum(axis=0).max())
    A0 = gen(nrm0)
    A = [gen(nrmj) for _ in range(nu)]
    x0 = np.linalg.qr(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))[0]
    xt = np.linalg.qr(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))[0]
    prob = systems.Problem("gue", A0, A, x0, xt, float(m), Nt, "fp64")
    return prob, rng.uniform(-1.0, 1.0, size=(2, nu, Nt))
