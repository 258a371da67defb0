"""The yardstick of the envelope gradient tests: a numpy restatement, never the code under test.

* adjoint(): the discrete adjoint of fixed-step Tsit5 on qoc_oracle's tableau.  FSAL is only a saving, so a step is a
  six-stage explicit Runge-Kutta with b = TSIT5_A[6]:
      X_i = x_n + h sum_{j<i} a_ij k_j,  k_i = A(t_i) X_i,  x_{n+1} = x_n + h sum_i b_i k_i,
  and with l = lambda_{n+1} (dJ = Re<lambda, dx>, qoc_oracle.compute_u_sensitivity), i = 6..1:
      kappa_i = h (b_i l + sum_{j>i} a_ji xi_j),  xi_i = A(t_i)^H kappa_i,
      dJ/dp_q += sum_j dc_j/dp_q(t_i) Re<kappa_i, A_j X_i>,  lambda_n = l + sum_i xi_i.
* dcdp(): analytic dc_j/dp_q(t) of the three pulses of src/parameterized_pulses.jl (d/dp_0 of DRAG and the sine basis
  with the integration horizon held fixed; the tunable bus on the branch of cos_envelope that t lies in).
* richardson_fd(): Richardson-extrapolated central differences of qoc_oracle.propagate_envelope.
"""
import math

import numpy as np

import qoc_oracle as O

ENVELOPES = {"tunable_bus": O.tunable_bus_envelope, "drag": O.drag_envelope, "sinebasis": O.sinebasis_envelope}
A_TAB = [np.array(r, dtype=float) for r in O.TSIT5_A]
C_TAB = O.TSIT5_C
B_TAB = A_TAB[6]


def transmon(N=4, anh=-0.3):
    """tests/test_gpu_ode.py::_transmon."""
    a = np.diag(np.sqrt(np.arange(1, N)), 1).astype(complex)
    ad = a.conj().T
    H0 = anh / 2 * (ad @ ad @ a @ a)
    return -1j * H0, [-1j * (a + ad) / 2, -1j * (1j * (ad - a)) / 2]


def tunable_bus_setup():
    """tests/test_gpu_ode.py::_tunable_bus_setup: (A0, [A1], x0 = |110>, target |200>, omega_Phi)."""
    from qoc_amd import systems as S
    H0, Hc, qb = S.tunable_bus_model()
    x0 = qb.columns(["110"])[:, 0].astype(complex)
    xt = qb.columns(["200"])[:, 0].astype(complex)
    i1, i2 = int(np.argmax(np.abs(x0))), int(np.argmax(np.abs(xt)))
    w_phi = abs(H0[i1, i1] - H0[i2, i2]) + (-0.002) * 2 * math.pi
    return -1j * H0, [-1j * Hc], x0, xt, w_phi


def dcdp(kind, p, t):
    """(nu, np) array of dc_j/dp_q(t)."""
    p = np.asarray(p, dtype=float)
    n = len(p)
    if kind == "tunable_bus":
        tp, trf, th0, w, amp = p[:5]
        d_tp = d_trf = 0.0
        if trf / 2 < t <= trf / 2 + tp:
            d = 1.0
        elif t <= trf / 2:
            a = 2 * math.pi * t / trf
            d = 0.5 * (1 - math.cos(a))
            d_trf = -0.5 * math.sin(a) * a / trf
        else:
            a = 2 * math.pi * (t - tp) / trf
            d = 0.5 * (1 - math.cos(a))
            d_tp = -0.5 * math.sin(a) * 2 * math.pi / trf
            d_trf = -0.5 * math.sin(a) * a / trf
        cw, sw = math.cos(w * t), math.sin(w * t)
        phi = math.pi * (th0 + amp * d * cw)
        c = math.sqrt(abs(math.cos(phi)))
        dc_dphi = -math.sin(phi) * math.copysign(1.0, math.cos(phi)) / (2 * c)
        out = np.zeros((1, n))
        out[0, :5] = dc_dphi * np.array([math.pi * amp * cw * d_tp, math.pi * amp * cw * d_trf, math.pi,
                                         -math.pi * amp * d * t * sw, math.pi * d * cw])
        return out
    if kind == "drag":
        tg, sg, amp, xi = p[:4]
        x, s2, s3 = t - tg / 2, sg ** 2, sg ** 3
        tmp, e0 = math.exp(-x * x / (2 * s2)), math.exp(-tg * tg / (8 * s2))
        out = np.zeros((2, n))
        out[0, :4] = [amp * (tmp * x / (2 * s2) + e0 * tg / (4 * s2)), amp * (tmp * x * x / s3 - e0 * tg * tg / (4 * s3)),
                      tmp - e0, 0.0]
        out[1, :4] = [amp * xi * tmp / (2 * s2) * (1 - x * x / s2), amp * xi * x * tmp / s3 * (2 - x * x / s2),
                      -xi * x / s2 * tmp, -amp * x / s2 * tmp]
        return out
    T = p[0]
    out = np.zeros((2, n))
    for k in range(1, n // 2 + 1):
        if 2 * k >= n:  # an even np: the last parameter has no partner (the kernel does not read it)
            break
        w = math.pi * k * t / T
        out[0, 2 * k - 1] = math.sin(w)
        out[1, 2 * k] = math.sin(w)
        out[0, 0] += p[2 * k - 1] * (-math.cos(w) * w / T)
        out[1, 0] += p[2 * k] * (-math.cos(w) * w / T)
    return out


def _gen(A0, A, cv):
    return A0 + sum(cv[j] * A[j] for j in range(len(A)))


def forward_states(A0, A, kind, p, x0, tgate, dt):
    """x_0 .. x_N of the plain six-stage scheme (no FSAL)."""
    env = ENVELOPES[kind]
    A0 = np.asarray(A0, dtype=complex)
    A = [np.asarray(a, dtype=complex) for a in A]
    nsteps = int(round(tgate / dt))
    xs = [np.array(x0, dtype=complex, copy=True)]
    for s in range(nsteps):
        x, t = xs[-1], s * dt
        ks = []
        for i in range(6):
            X = x + dt * sum(A_TAB[i][j] * ks[j] for j in range(i)) if i else x
            ks.append(_gen(A0, A, np.atleast_1d(env(p, t + C_TAB[i] * dt))) @ X)
        xs.append(x + dt * sum(B_TAB[j] * ks[j] for j in range(6)))
    return xs


def adjoint(A0, A, kind, p, x0, tgate, dt, dJ_dx):
    """(x(tgate), dJ/dp) by the discrete adjoint; dJ_dx: x(tgate) -> lambda_N."""
    env = ENVELOPES[kind]
    A0 = np.asarray(A0, dtype=complex)
    A = [np.asarray(a, dtype=complex) for a in A]
    p = np.asarray(p, dtype=float)
    xs = forward_states(A0, A, kind, p, x0, tgate, dt)
    lam = np.asarray(dJ_dx(xs[-1]), dtype=complex).reshape(xs[-1].shape)
    g = np.zeros(len(p))
    h = dt
    for s in range(len(xs) - 2, -1, -1):
        x, t = xs[s], s * dt
        ks, Xs, gens = [], [], []
        for i in range(6):
            X = x + h * sum(A_TAB[i][j] * ks[j] for j in range(i)) if i else x
            M = _gen(A0, A, np.atleast_1d(env(p, t + C_TAB[i] * h)))
            Xs.append(X)
            gens.append(M)
            ks.append(M @ X)
        xi = [None] * 6
        new = lam.copy()
        for i in range(5, -1, -1):
            kap = h * (B_TAB[i] * lam + sum(A_TAB[j][i] * xi[j] for j in range(i + 1, 6)))
            xi[i] = gens[i].conj().T @ kap
            sj = np.array([np.real(np.sum(np.conj(kap) * (Aj @ Xs[i]))) for Aj in A])
            g += dcdp(kind, p, t + C_TAB[i] * h).T @ sj
            new = new + xi[i]
        lam = new
    return xs[-1], g


def trace_cost(x_target, n):
    """(J, dJ_dx) of qoc_oracle.setup_infidelity for 1-D or 2-D states."""
    Xt = np.asarray(x_target, dtype=complex)
    J2, dJ2 = O.setup_infidelity(Xt, n)

    def J(x):
        return J2(x if x.ndim == 2 else x[:, None])

    def dJ(x):
        return dJ2(x if x.ndim == 2 else x[:, None]).reshape(x.shape)
    return J, dJ


def richardson_fd(A0, A, kind, p, x0, tgate, dt, J, rel_step=1e-5):
    """dJ/dp by (4 D(h/2) - D(h)) / 3, D the central difference of J(propagate_envelope), h = rel_step max(1, |p_q|);
    tgate (the horizon) is held fixed.  The step is small because the scheme's J is only C^1 in the tunable bus's
    t_rise_fall and t_plateau (a stage time crosses from one branch of cos_envelope to the next), where the
    extrapolation gains nothing and the error is O(h); round-off, eps / h ~ 1e-11, stays below that."""
    env = ENVELOPES[kind]
    p = np.asarray(p, dtype=float)

    def f(pp):
        return J(O.propagate_envelope(A0, A, env, pp, x0, tgate, dt))

    def D(q, h):
        e = np.zeros(len(p))
        e[q] = h
        return (f(p + e) - f(p - e)) / (2 * h)
    g = np.zeros(len(p))
    for q in range(len(p)):
        h = rel_step * max(1.0, abs(p[q]))
        g[q] = (4 * D(q, h / 2) - D(q, h)) / 3
    return g


# the four cases of the reference's own check (system, kind, p, tgate, dt)
def case(name):
    if name == "tunable_bus":
        A0, A, x0, xt, w = tunable_bus_setup()
        return A0, A, x0, xt, 1, "tunable_bus", np.array([2.0, 1.5, 0.25, w, 0.13]), 3.5, 2e-3
    A0, A = transmon()
    x0 = np.eye(4, dtype=complex)[:, :2]
    xt = np.eye(4, dtype=complex)[:, [1, 0]]
    if name == "drag":
        return A0, A, x0, xt, 2, "drag", np.array([20.0, 5.0, 0.16, 0.4]), 20.0, 0.05
    if name == "drag_coarse":
        return A0, A, x0, xt, 2, "drag", np.array([20.0, 5.0, 0.16, 0.4]), 20.0, 0.5
    return A0, A, x0, xt, 2, "sinebasis", np.array([20.0, 0.05, 0.01, -0.02, 0.03, 0.004, 0.0]), 20.0, 0.05
