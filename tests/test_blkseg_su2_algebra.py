"""The recurrences of the segmented eval's phase-free fast path (csrc/qoc_blkseg.hpp: sk2_form_v, sk2_vmul, the z^Nt
of x_N, the Ĝ = z̄ G recursion of phase 3 and the traces from m1, m2 alone), restated in numpy on random 2-row blocks
with zero-diagonal controls, against scipy.linalg.expm products and the matrix recurrence for
M = Σ_{a+b<ORD} X^b K X^a / (a+b+1)!  (exact: ∫_0^1 e^{sX} K e^{(1-s)X} ds, scipy's expm_frechet).

A slice of the lane's block is A_k = i m0 I + Ã_0 + u_1 A_1 + u_2 A_2 with Ã_0 = [[i d0, r0 + i q0], [-r0 + i q0, i d1]]
and A_j = [[0, r_j + i q_j], [-r_j + i q_j, 0]]; t = (d0 + d1) / 2, a = (d0 - d1) / 2, z = e^{i (m0 + t)}, and
exp(A_k) = z V_k, V_k = [[α, β], [-β̄, ᾱ]], α = cos ω + i sinc ω a, β = sinc ω (r + i q), ω² = a² + r² + q².
Bar 1e-13 (absolute, on unitary factors and on traces of O(1) operands), spectral half-widths up to 0.9 and up to
1000 slices.
"""
import math

import numpy as np
import pytest
import scipy.linalg as sl

BAR = 1e-13
KMAX = 9  # the kernel's longest series (terms up to ω^19)
_C = [(-1.0) ** k / math.factorial(2 * k) for k in range(KMAX + 1)]
_S = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(KMAX + 1)]
_D = [(-1.0) ** k * 2 * (k + 1) / math.factorial(2 * k + 3) for k in range(KMAX + 1)]


def _horner(c, w):
    s = 0.0
    for v in reversed(c):
        s = s * w + v
    return s


def _sk(d0, d1, r, q):
    return np.array([[1j * d0, r + 1j * q], [-r + 1j * q, 1j * d1]])


class Block:
    """One random block: Ã_0 with a diagonal, two zero-diagonal controls, a scalar shift i m0, half-width <= rho."""

    def __init__(self, rng, rho, n):
        self.m0 = rng.uniform(-0.3, 0.3)
        g = rng.uniform(-1, 1, size=(3, 4))
        g[1:, :2] = 0.0  # controls: zero diagonals
        umax = 1.0
        # ω <= |a| + |(r0, q0)| + umax (|(r1, q1)| + |(r2, q2)|) <= rho
        bound = abs(g[0, 0] - g[0, 1]) / 2 + np.hypot(*g[0, 2:]) + umax * (np.hypot(*g[1, 2:]) + np.hypot(*g[2, 2:]))
        self.g = g * (rho / bound)
        self.m0 *= rho
        self.u = rng.uniform(-umax, umax, size=(n, 2))
        self.t = 0.5 * (self.g[0, 0] + self.g[0, 1])
        self.a = 0.5 * (self.g[0, 0] - self.g[0, 1])
        self.z = np.exp(1j * self.m0) * np.exp(1j * self.t)

    def A(self, j):
        return _sk(*self.g[j]) + (1j * self.m0 * np.eye(2) if j == 0 else 0)

    def X(self, k):
        return self.A(0) + self.u[k, 0] * self.A(1) + self.u[k, 1] * self.A(2)

    def rq(self, k):
        r = self.g[0, 2] + self.u[k, 0] * self.g[1, 2] + self.u[k, 1] * self.g[2, 2]
        q = self.g[0, 3] + self.u[k, 0] * self.g[1, 3] + self.u[k, 1] * self.g[2, 3]
        return r, q

    def v(self, k):
        """sk2_form_v: (α, β) and the series values [cos ω, sinc ω, s3]."""
        r, q = self.rq(k)
        w = self.a * self.a + r * r + q * q
        cw, sw, s3 = _horner(_C, w), _horner(_S, w), _horner(_D, w)
        return complex(cw, sw * self.a), complex(sw * r, sw * q), (cw, sw, s3)


def _mat(p, y):
    return np.array([[p, y], [-np.conj(y), np.conj(p)]])


def _zpow(z, n):
    """z^n by square-and-multiply, as the kernel forms z^Nt."""
    w, b = 1.0 + 0j, z
    while n > 0:
        if n & 1:
            w = w * b
        b = b * b
        n >>= 1
    return w


def _zpow_ref(z, n):
    """The same power of the same (rounded) z in extended precision."""
    w, b = np.clongdouble(1.0), np.clongdouble(z)
    for _ in range(n):
        w = w * b
    return w


CASES = [(rho, n, seed) for rho in (0.05, 0.24, 0.66, 0.9) for n, seed in ((11, 1), (37, 2), (1000, 3))]


@pytest.mark.parametrize("rho,n,seed", CASES)
def test_v_and_segment_product(rho, n, seed):
    """z V_k against expm(A_k) for every slice, and z^n (p, y) against the product of the exponentials."""
    blk = Block(np.random.default_rng(1000 * seed + int(100 * rho)), rho, n)
    p, y = 1.0 + 0j, 0j
    ref = np.eye(2, dtype=complex)
    worst = 0.0
    for k in range(n):
        al, be, _ = blk.v(k)
        U = sl.expm(blk.X(k))
        worst = max(worst, np.abs(blk.z * _mat(al, be) - U).max())
        p, y = al * p - be * np.conj(y), al * y + be * np.conj(p)  # sk2_vmul
        ref = U @ ref
    assert worst <= BAR, worst
    err = np.abs(_zpow(blk.z, n) * _mat(p, y) - ref).max()
    print("rho", rho, "n", n, "slice", worst, "product", err)
    assert err <= BAR, err


@pytest.mark.parametrize("n", [1, 2, 5, 37, 50, 999, 1000])
def test_zpow_square_and_multiply(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        z = np.exp(1j * rng.uniform(-0.9, 0.9))
        err = abs(np.clongdouble(_zpow(z, n)) - _zpow_ref(z, n))
        assert err <= BAR, (n, float(err))


@pytest.mark.parametrize("rho,n,seed", CASES)
def test_ghat_recursion(rho, n, seed):
    """Phase 3 on Ĝ = z̄ G: K_k = V_k^H Ĝ_{k+1} is the parent's U_k^H G_{k+1}, and Ĝ_k = K_k V_k stays z̄ G_k."""
    rng = np.random.default_rng(2000 * seed + int(100 * rho))
    blk = Block(rng, rho, n)
    G = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    G /= np.abs(G).max()
    Gh = np.conj(blk.z) * G
    eK = eG = 0.0
    for k in range(n - 1, -1, -1):
        al, be, _ = blk.v(k)
        V = _mat(al, be)
        U = sl.expm(blk.X(k))
        K = V.conj().T @ Gh
        Kref = U.conj().T @ G
        Gh = K @ V
        G = Kref @ U
        eK = max(eK, np.abs(K - Kref).max())
        eG = max(eG, np.abs(Gh - np.conj(blk.z) * G).max())
    print("rho", rho, "n", n, "K", eK, "G", eG)
    assert eK <= BAR and eG <= BAR, (eK, eG)


def _pauli2(K):
    """Doubled Pauli components of K: (2 Re k, 2 Im k)."""
    k = np.array([K[0, 0] + K[1, 1], K[0, 1] + K[1, 0], 1j * (K[0, 1] - K[1, 0]), K[0, 0] - K[1, 1]])
    return k.real, k.imag


def _traces_m12(blk, k, K, order):
    """Re tr(A_j M), j = 1, 2, from m1 and m2 alone (sk2_contract_pauli / sk2_contract_exact under CX)."""
    kr, ki = _pauli2(K)
    r, q = blk.rq(k)
    x0, x1, x2, x3 = blk.m0 + blk.t, q, r, blk.a
    if order == 1:
        m1, m2 = ki[1], ki[2]
    elif order == 2:
        m1 = ki[1] + x0 * kr[1] + kr[0] * x1
        m2 = ki[2] + x0 * kr[2] + kr[0] * x2
    elif order == 3:
        di = x1 * ki[1] + x2 * ki[2] + x3 * ki[3]
        w = x1 * x1 + x2 * x2 + x3 * x3
        al1 = 1.0 - 0.5 * x0 * x0 - w / 6.0
        c = kr[0] - x0 * ki[0] - di / 3.0
        m1 = al1 * ki[1] + x0 * kr[1] + c * x1
        m2 = al1 * ki[2] + x0 * kr[2] + c * x2
    else:  # exact
        _, _, (cw, sw, s3) = blk.v(k)
        dr = x1 * kr[1] + x2 * kr[2] + x3 * kr[3]
        di = x1 * ki[1] + x2 * ki[2] + x3 * ki[3]
        cr, ci = -(sw * ki[0] + s3 * dr), sw * kr[0] - s3 * di
        zr, zi = blk.z.real, blk.z.imag
        m1 = zr * (sw * ki[1] + ci * x1) + zi * (sw * kr[1] + cr * x1)
        m2 = zr * (sw * ki[2] + ci * x2) + zi * (sw * kr[2] + cr * x2)
    out = []
    for j in (1, 2):
        a1, a2 = 2.0 * blk.g[j, 3], 2.0 * blk.g[j, 2]  # the control's doubled Pauli vector: components 0 and 3 vanish
        out.append(-0.5 * (a1 * m1 + a2 * m2))
    return out


def _traces_ref(blk, k, K, order):
    X = blk.X(k)
    if order == "exact":
        M = sl.expm_frechet(X, K, compute_expm=False)
    else:
        M = np.zeros((2, 2), complex)
        for a in range(order):
            for b in range(order - a):
                M += np.linalg.matrix_power(X, b) @ K @ np.linalg.matrix_power(X, a) / math.factorial(a + b + 1)
    return [np.trace(blk.A(j) @ M).real for j in (1, 2)]


@pytest.mark.parametrize("order", [1, 2, 3, "exact"])
@pytest.mark.parametrize("rho", [0.05, 0.24, 0.66, 0.9])
def test_traces_from_m1_m2(rho, order):
    rng = np.random.default_rng(int(1000 * rho) + (0 if order == "exact" else order))
    blk = Block(rng, rho, 11)
    worst = 0.0
    for k in range(11):
        K = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
        K /= np.abs(K).max()
        got = _traces_m12(blk, k, K, order)
        ref = _traces_ref(blk, k, K, order)
        worst = max(worst, max(abs(g - r) for g, r in zip(got, ref)))
    print("rho", rho, "order", order, worst)
    assert worst <= BAR, worst
