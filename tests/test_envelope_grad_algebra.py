"""Pins the numpy yardstick of the envelope gradient (tests/envgrad_util.py) on the CPU: its forward states are the
oracle's, its gradient is the Richardson-extrapolated finite difference of qoc_oracle.propagate_envelope, and its
analytic envelope derivatives are differences of the oracle's envelopes.  No engine code runs here.

The finite difference is the limiting side of the 1e-8 bound: the worst of the four cases is the tunable bus
(|H| ~ 104 rad/ns, 1750 steps), where it carries about 4e-10 itself; the DRAG row at dt = 0.5 shows that the formulas
are the derivative of the scheme, not of the ODE (the scheme's J is far from the ODE's there).
"""
import math

import numpy as np
import pytest

import envgrad_util as E
import qoc_oracle as O

CASES = ["drag", "drag_coarse", "sinebasis", "tunable_bus"]


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in CASES:
        A0, A, x0, xt, n, kind, p, tgate, dt = E.case(name)
        J, dJ = E.trace_cost(xt, n)
        xN, g = E.adjoint(A0, A, kind, p, x0, tgate, dt, dJ)
        out[name] = (xN, g)
    return out


@pytest.mark.parametrize("name", CASES)
def test_forward_states_equal_oracle(refs, name):
    A0, A, x0, xt, n, kind, p, tgate, dt = E.case(name)
    xr = O.propagate_envelope(A0, A, E.ENVELOPES[kind], p, x0, tgate, dt)
    err = np.abs(refs[name][0] - xr).max()
    print(name, "max |x - x_oracle| =", err)
    assert err <= 1e-13


@pytest.mark.parametrize("name", CASES)
def test_adjoint_matches_richardson_fd(refs, name):
    A0, A, x0, xt, n, kind, p, tgate, dt = E.case(name)
    J, _ = E.trace_cost(xt, n)
    g = refs[name][1]
    gfd = E.richardson_fd(A0, A, kind, p, x0, tgate, dt, J)
    err = np.linalg.norm(g - gfd) / np.linalg.norm(gfd)
    print(name, "g =", g, "rel err vs FD =", err)
    assert err <= 1e-8


def _fd_env(kind, p, t, q, h):
    env = E.ENVELOPES[kind]
    e = np.zeros(len(p))

    def D(hh):
        e[:] = 0
        e[q] = hh
        return (np.atleast_1d(env(p + e, t)) - np.atleast_1d(env(p - e, t))) / (2 * hh)
    return (4 * D(h / 2) - D(h)) / 3


@pytest.mark.parametrize("kind,p,ts", [
    ("drag", np.array([20.0, 5.0, 0.16, 0.4]), [0.0, 3.3, 10.0, 17.9]),
    ("sinebasis", np.array([20.0, 0.05, 0.01, -0.02, 0.03, 0.004, 0.0]), [0.7, 9.1, 19.5]),
    # cos_envelope's three branches for t_plateau = 2, t_rise_fall = 1.5: rise (t <= 0.75), plateau, fall
    ("tunable_bus", np.array([2.0, 1.5, 0.25, 4.1, 0.13]), [0.31, 1.9, 3.2]),
])
def test_analytic_envelope_derivatives(kind, p, ts):
    for t in ts:
        an = E.dcdp(kind, p, t)
        for q in range(len(p)):
            fd = _fd_env(kind, p, t, q, 1e-3 * max(1.0, abs(p[q])))
            assert np.abs(an[:, q] - fd).max() <= 1e-9 * max(1.0, np.abs(fd).max()), (kind, t, q, an[:, q], fd)
    if kind == "tunable_bus":  # the three t above do lie in the three branches
        tp, trf = p[0], p[1]
        assert ts[0] <= trf / 2 < ts[1] <= trf / 2 + tp < ts[2]
        assert O.cos_envelope(tp, trf, ts[1]) == 1.0 and 0 < O.cos_envelope(tp, trf, ts[2]) < 1
