"""Phase 3 of the segmented eval's phase-free fast path in the Pauli basis (csrc/qoc_blkseg.hpp: sk2_pauli_of,
sk2_pauli_k, sk2_pauli_rot, sk2_contract_pauli_k and the time-scale trace), restated in numpy against the matrix
products they replace.

V = v0 I + i n.σ in SU(2) (sk2_form_v's v = (v0, n3, n2, n1), n = sinc ω (q, r, a)), Ĝ = g0 I + g.σ with complex g0
and g, carried doubled; d = n.g, t = n x g:
  K = V^H Ĝ:    k0 = v0 g0 - i d,  k = v0 g - i g0 n + t
  Ĝ' = V^H Ĝ V: g0' = g0,  g' = g + 2 (v0 t + n x t)
Bars: 1e-14 absolute on K and Ĝ' (operands of modulus <= 1, a dozen roundings each), 1e-13 on the traces (the bar of
tests/test_blkseg_su2_algebra.py); the drift of the rotation recursion over 1000 steps may not exceed the matrix
recursion's, both measured here against an extended-precision recursion.
"""
import math

import numpy as np
import pytest

SIG = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], complex), np.array([[0, -1j], [1j, 0]]),
       np.array([[1, 0], [0, -1]], complex)]
_C = [(-1.0) ** k / math.factorial(2 * k) for k in range(6)]  # the K = 5 series (ρ <= 0.24)
_S = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(6)]


def _horner(c, w):
    s = 0.0
    for v in reversed(c):
        s = s * w + v
    return s


def _v(x):
    """sk2_form_v on the Pauli vector x = (q, r, a) of Â - i t I: (v0, n) = (cos ω, sinc ω x) from the series in ω²."""
    w = x @ x
    return _horner(_C, w), _horner(_S, w) * x


def _vmat(v0, n):
    return v0 * SIG[0] + 1j * (n[0] * SIG[1] + n[1] * SIG[2] + n[2] * SIG[3])


def _pauli_of(G):
    """sk2_pauli_of: the doubled components (2 g0, 2 g) of a 2 x 2 matrix."""
    return G[0, 0] + G[1, 1], np.array([G[0, 1] + G[1, 0], 1j * (G[0, 1] - G[1, 0]), G[0, 0] - G[1, 1]])


def _mat_of(g0, g):
    return 0.5 * (g0 * SIG[0] + g[0] * SIG[1] + g[1] * SIG[2] + g[2] * SIG[3])


def _pauli_k(v0, n, g0, g):
    """sk2_pauli_k: t = n x g and K = V^H Ĝ's components (k0, k)."""
    t = np.cross(n, g)
    return t, v0 * g0 - 1j * (n @ g), v0 * g - 1j * g0 * n + t


def _pauli_rot(v0, n, t, g):
    """sk2_pauli_rot: g' = g + 2 (v0 t + n x t)."""
    return g + (2 * v0) * t + np.cross(2 * n, t)


def _blocks(seed, rho, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        x = rng.standard_normal(3)
        x *= rng.uniform(0.0, rho) / np.linalg.norm(x)
        G = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
        yield rng, x, G / np.abs(G).max()


@pytest.mark.parametrize("rho", [0.05, 0.24, 0.66, 0.9])
def test_k_and_rotation(rho):
    """K's components and the rotated Ĝ of random skew Â and complex G against V^H G and V^H G V."""
    eK = eG = e0 = 0.0
    for _, x, G in _blocks(int(100 * rho), rho, 200):
        w = x @ x
        v0, n = math.cos(math.sqrt(w)), np.sinc(math.sqrt(w) / np.pi) * x  # (beyond K = 5's radius: the closed form)
        V = _vmat(v0, n)
        g0, g = _pauli_of(G)
        t, k0, k = _pauli_k(v0, n, g0, g)
        K0, Kv = _pauli_of(V.conj().T @ G)
        eK = max(eK, abs(k0 - K0), np.abs(k - Kv).max())
        R0, Rv = _pauli_of(V.conj().T @ G @ V)
        e0 = max(e0, abs(g0 - R0))  # g0 is not touched
        eG = max(eG, np.abs(_pauli_rot(v0, n, t, g) - Rv).max())
    print("rho", rho, "K", eK, "g0", e0, "g", eG)
    assert eK <= 1e-14 and e0 <= 1e-14 and eG <= 1e-14, (eK, e0, eG)


def _traces_pauli(order, x0, x, a, k0, k):
    """sk2_contract_pauli_k: Re tr(A_j M) from K's doubled components, A_j = i a_j.σ with a_j[3] = 0 (zero-diagonal
    controls), X = i (x0 I + x.σ).  Order 1 reads Im k1, Im k2; order 2 also Re k0, Re k1, Re k2; order 3 also Im k0, Im k3."""
    if order == 1:
        m = k.imag[:2]
    elif order == 2:
        m = k.imag[:2] + x0 * k.real[:2] + k0.real * x[:2]
    else:
        di = x @ k.imag
        al1 = 1.0 - 0.5 * x0 * x0 - (x @ x) / 6.0
        c = k0.real - x0 * k0.imag - di / 3.0
        m = al1 * k.imag[:2] + x0 * k.real[:2] + c * x[:2]
    return [-0.5 * (2.0 * aj[:2]) @ m for aj in a]


def _traces_matrix(order, X, A, K):
    """sk2_contract's matrix recurrence: M = Σ_{a+b<order} X^b K X^a / (a+b+1)!, Re tr(A_j M)."""
    M = np.zeros((2, 2), complex)
    for p in range(order):
        for q in range(order - p):
            M += np.linalg.matrix_power(X, q) @ K @ np.linalg.matrix_power(X, p) / math.factorial(p + q + 1)
    return [np.trace(Aj @ M).real for Aj in A]


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("rho", [0.05, 0.24, 0.66, 0.9])
def test_contraction_from_components(rho, order):
    """The order-1/2/3 traces from the components sk2_pauli_k forms, against the matrix recurrence on K = V^H G."""
    worst = 0.0
    for rng, x, G in _blocks(int(1000 * rho) + order, rho, 50):
        x0 = rng.uniform(-rho, rho)  # the block's mean diagonal with the shift Im μ_0
        a = rng.uniform(-1, 1, size=(2, 3))
        a[:, 2] = 0.0
        w = x @ x
        v0, n = math.cos(math.sqrt(w)), np.sinc(math.sqrt(w) / np.pi) * x
        _, k0, k = _pauli_k(v0, n, *_pauli_of(G))
        X = 1j * (x0 * SIG[0] + x[0] * SIG[1] + x[1] * SIG[2] + x[2] * SIG[3])
        A = [1j * (aj[0] * SIG[1] + aj[1] * SIG[2]) for aj in a]
        got = _traces_pauli(order, x0, x, a, k0, k)
        ref = _traces_matrix(order, X, A, _vmat(v0, n).conj().T @ G)
        worst = max(worst, max(abs(p - q) for p, q in zip(got, ref)))
    print("rho", rho, "order", order, worst)
    assert worst <= 1e-13, worst


def test_time_scale_trace():
    """tr(X Ĝ) = i (x0 2 g0 + x . 2 g) on the doubled components."""
    worst = 0.0
    for rng, x, G in _blocks(7, 0.9, 200):
        x0 = rng.uniform(-0.9, 0.9)
        g0, g = _pauli_of(G)
        X = 1j * (x0 * SIG[0] + x[0] * SIG[1] + x[1] * SIG[2] + x[2] * SIG[3])
        worst = max(worst, abs(1j * (x0 * g0 + x @ g) - np.trace(X @ G)))
    print(worst)
    assert worst <= 1e-14, worst


@pytest.mark.parametrize("steps", [42, 1000])
def test_rotation_drift(steps):
    """Ĝ over `steps` slices with K = 5 series values at ρ <= 0.24 in random directions: the rotation recursion and the
    matrix recursion Ĝ <- (V^H Ĝ) V in fp64, each against the matrix recursion in extended precision on the exact
    V = exp(Â - i t I) (cos and sinc there, not the series: at ω = 0.24 the K = 5 series stops 8e-17 short of cos ω, always
    to the same side, which the matrix form accumulates in |Ĝ| and the rotation, which uses |V| = 1, does not), as max
    relative error of Ĝ.  Over 1000 steps the rotation may not be worse than the matrix form; over 42 steps, where the
    two are a few roundings apart either way, it stays within one rounding unit (2^-52 rounded up) per step."""
    rng = np.random.default_rng(steps)
    L = np.longdouble
    xs = rng.standard_normal((steps, 3))
    xs *= (rng.uniform(0.02, 0.24, size=steps) / np.linalg.norm(xs, axis=1))[:, None]
    G = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    G /= np.abs(G).max()
    Gm = G.copy()
    g0, g = _pauli_of(G)
    Gt = G.astype(np.clongdouble)
    sig = [s.astype(np.clongdouble) for s in SIG]
    for x in xs:
        v0, n = _v(x)
        t, _, _ = _pauli_k(v0, n, g0, g)
        g = _pauli_rot(v0, n, t, g)
        V = _vmat(v0, n)
        Gm = (V.conj().T @ Gm) @ V
        xt = x.astype(L)
        om = np.sqrt(xt @ xt)
        v0t, nt = np.cos(om), np.sin(om) / om * xt
        Vt = v0t * sig[0] + np.clongdouble(1j) * (nt[0] * sig[1] + nt[1] * sig[2] + nt[2] * sig[3])
        Gt = (Vt.conj().T @ Gt) @ Vt
    scale = float(np.abs(Gt).max())
    e_rot = float(np.abs(_mat_of(g0, g).astype(np.clongdouble) - Gt).max()) / scale
    e_mat = float(np.abs(Gm.astype(np.clongdouble) - Gt).max()) / scale
    print("steps", steps, "rotation", e_rot, "matrix", e_mat)
    assert e_mat < 1e-12  # (the truth is one: both stay at rounding level)
    if steps >= 1000:
        assert e_rot <= e_mat, (e_rot, e_mat)
    else:  # 42 steps (a segment of the flagship shape): both a few roundings, neither ahead of the other reliably
        assert e_rot <= 42 * 2.3e-16, e_rot
