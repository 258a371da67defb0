"""The phase-free fast path of the segmented block eval (csrc/qoc_blkseg.hpp: blocks of 2 rows whose control blocks
have zero diagonals and no shifts, the cavity's class).  The slice loops run on V_k = U_k / z in SU(2) (4 reals), the
constant phase z of a block enters once per lane: z^Nt on x_N (square-and-multiply) and z̄ on G at the segment's end;
the traces take m1, m2 alone.  Against oracle/qoc_oracle.grape_eval at the bars of tests/test_gpu_blkseg.py:
|ΔJ| <= 1e-12 and ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed.  Shape: cavity, N_cavity = 10 (10 blocks of 2 rows), B = 3.
"""
import dataclasses
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import MU, assert_seed as _assert_seed, engine as _engine, eval_dev, split_dev

pytestmark = pytest.mark.gpu

PEN = ([16, 17, 18, 19, 5], [0, 1], MU)  # tests/test_gpu_blkseg_penalty.py, cavity20


def _eval_dev(e, u, order=3):
    out = eval_dev(e, u, order)
    assert e.info()["backward"] == "segmented", e.info()
    return out


def _split_dev(e, u, order=3):
    out = split_dev(e, u, order)
    info = e.info()
    assert info["split_forward"] == "segmented" and info["backward"] == "segmented", info
    return out


@functools.lru_cache(maxsize=None)
def _case(Nt, amp=1.0, B=3):
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=Nt)  # N = 20, 10 blocks of 2, m = 2
    return p, systems.cavity_controls(B, Nt, seed=82 + Nt) * amp


@functools.lru_cache(maxsize=None)
def _oracle(Nt, amp=1.0, order=3, pen=False):
    """The oracle's (J, dJdu) of every seed of a case: computed once, shared, never changed."""
    prob, u = _case(Nt, amp)
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=order,
                              penalty=PEN if pen else None)[:2] for b in range(u.shape[0]))


def _check(prob, u, J, g, ref, tag):
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], tag + (b,))


@pytest.mark.parametrize("Nt,S", [(50, None), (37, 7), (37, 8), (5, 7)])
def test_su2_segment_shapes(built_lib, monkeypatch, Nt, S):
    """Nt = 50 with the default segment count; Nt = 37 capped at 7 segments (L = 6, the last segment one slice long:
    its pair of phase 1 runs the select variant, and z^37 has both kinds of bits) and at 8 (L = 5, odd: every
    segment's last pair is half empty, the last segment has 2 slices); Nt = 5: fewer slices than segments."""
    prob, u = _case(Nt)
    e = _engine(prob, 3, monkeypatch, S=S)
    J, g = _eval_dev(e, u)
    e.close()
    _check(prob, u, J, g, _oracle(Nt), (Nt, S))


def test_su2_single_seed(built_lib, monkeypatch):
    prob, u = _case(50)
    e = _engine(prob, 1, monkeypatch)
    J, g = _eval_dev(e, u[:1])
    e.close()
    _check(prob, u[:1], J, g, _oracle(50), ("B1",))


@pytest.mark.parametrize("amp", [1.0, 8.0, 14.0])
def test_su2_series_degree_classes(built_lib, monkeypatch, amp):
    """The series classes K = 5, 7, 9 (ρ = 0.154 + 0.05 amp at |u| = 0.05 amp per control), as
    tests/test_gpu_blkseg.py::test_segmented_series_degree_classes moves through them."""
    prob, u = _case(40, amp)
    e = _engine(prob, 3, monkeypatch)
    J, g = _eval_dev(e, u)
    e.close()
    _check(prob, u, J, g, _oracle(40, amp), (amp,))


@pytest.mark.parametrize("order", [1, 2, 3, 4, "exact"])
def test_su2_gradient_orders(built_lib, monkeypatch, order):
    """Orders 1..3 (the traces from m1, m2 alone), 4 (the matrix recurrence on the same K) and the exact gradient
    against the oracle's exact one (tests/test_gpu_blkseg_exact.py)."""
    prob, u = _case(50)
    e = _engine(prob, 3, monkeypatch)
    J, g = _eval_dev(e, u, order)
    e.close()
    _check(prob, u, J, g, _oracle(50, order=order), (order,))


@pytest.mark.parametrize("order", [3, "exact"])
def test_su2_split_form_bitwise(built_lib, monkeypatch, order):
    """propagate_device + grape_sensitivity_device (G through HBM, z̄ applied by the backward launch) bitwise the
    fused eval, at Nt = 37 in 7 segments."""
    prob, u = _case(37)
    e = _engine(prob, 3, monkeypatch, S=7)
    J, g = _split_dev(e, u, order)
    Jf, gf = _eval_dev(e, u, order)
    e.close()
    assert np.array_equal(J, Jf) and np.array_equal(g, gf)
    _check(prob, u, J, g, _oracle(37, order=order), ("split", order))


def test_su2_penalised(built_lib, monkeypatch):
    """The guard-state penalty on the same path (the source of λ_k turned by z̄): against the oracle's penalised
    values, the fused and the split form bitwise equal."""
    prob, u = _case(50)
    e = _engine(prob, 3, monkeypatch, pen=PEN)
    J, g = _eval_dev(e, u)
    Js, gs = _split_dev(e, u)
    e.close()
    assert np.array_equal(J, Js) and np.array_equal(g, gs)
    _check(prob, u, J, g, _oracle(50, pen=True), ("pen",))


@pytest.mark.parametrize("which", ["control_diagonal", "a0_shift"])
def test_su2_neighbouring_classes(built_lib, monkeypatch, which):
    """Generators just outside or at the edge of the class, kept exactly skew-Hermitian: one control with a nonzero
    diagonal entry (not zero-diagonal: the general 2-row form runs), and A0 shifted by a multiple of i I (the shift
    moves into z)."""
    prob, u = _case(37)
    if which == "control_diagonal":
        D = np.zeros(prob.N)
        D[3] = 0.04
        prob = dataclasses.replace(prob, A=[prob.A[0] + 1j * np.diag(D), prob.A[1]])
    else:
        prob = dataclasses.replace(prob, A0=prob.A0 + 0.21j * np.eye(prob.N))
    for M in [prob.A0] + list(prob.A):
        assert np.array_equal(M, -M.conj().T)
    e = _engine(prob, 3, monkeypatch, S=7)
    J, g = _eval_dev(e, u)
    e.close()
    for b in range(3):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3)
        _assert_seed(J[b], g[b], J0, g0, (which, b))


def test_su2_known_answer_diagonal_drift(built_lib, monkeypatch):
    """A0 = i diag(d) under zero control amplitudes: x_N = e^{i d Nt} x_0 row by row, so J has a closed form.  This
    pins z^Nt, which no G-based quantity sees."""
    prob, u = _case(37)
    rng = np.random.default_rng(5)
    d = rng.uniform(-0.2, 0.2, size=prob.N)
    prob = dataclasses.replace(prob, A0=1j * np.diag(d))
    u = np.zeros_like(u)
    e = _engine(prob, 3, monkeypatch, S=7)
    J, g = _eval_dev(e, u)
    e.close()
    xN = np.exp(1j * d * prob.Nt)[:, None] * prob.x0
    Jc = 1.0 - abs(np.trace(prob.x_target.conj().T @ xN)) ** 2 / prob.n ** 2
    J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[0], prob.x0, prob.x_target, prob.n, order=3)
    print("closed form", Jc, "oracle", J0, "gpu", J[0], "dJ", J[0] - Jc)
    assert 0.05 < Jc < 0.999  # the phases matter to J
    for b in range(3):
        assert abs(J[b] - Jc) <= 1e-12, (b, J[b] - Jc)
        _assert_seed(J[b], g[b], J0, g0, ("diag", b))
