"""Phase 3 of the phase-free fast path in the Pauli basis (csrc/qoc_blkseg.hpp: sk2_pauli_k, sk2_pauli_rot,
sk2_contract_pauli_k; blocks of 2 rows with zero-diagonal controls, orders 1..3, no penalty).  Ĝ = z̄ G is carried as
its doubled Pauli components and rotated, g' = g + 2 (v0 t + n x t), instead of multiplied as a matrix; K's components
come from the same t = n x g.  Against oracle/qoc_oracle.grape_eval at the bars of tests/test_gpu_blkseg.py:
|ΔJ| <= 1e-12 and ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed.  Shape: cavity, N_cavity = 10 (10 blocks of 2 rows), B = 3.
"""
import dataclasses
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import assert_seed as _assert_seed, engine as _engine, eval_dev, split_dev

pytestmark = pytest.mark.gpu


def _eval_dev(e, u, order=3):
    out = eval_dev(e, u, order)
    assert e.info()["backward"] == "segmented", e.info()
    return out


@functools.lru_cache(maxsize=None)
def _case(Nt, amp=1.0):
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=Nt)  # N = 20, 10 blocks of 2, m = 2
    return p, systems.cavity_controls(3, Nt, seed=182 + Nt) * amp


@functools.lru_cache(maxsize=None)
def _oracle(Nt, amp=1.0, order=3):
    """The oracle's (J, dJdu) of every seed of a case: computed once, shared, never changed."""
    prob, u = _case(Nt, amp)
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=order)[:2]
                 for b in range(u.shape[0]))


def _check(u, J, g, ref, tag):
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], tag + (b,))


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("Nt,S", [(37, 7), (37, 8), (5, 7), (50, None)])
def test_pauli_segment_shapes(built_lib, monkeypatch, Nt, S, order):
    """Nt = 37 capped at 7 segments (L = 6: the last segment is one slice long, so the other lanes run select steps
    with their six reals held) and at 8 (L = 5, the last segment two slices); Nt = 5: fewer slices than segments;
    Nt = 50 with the default segment count.  Each at the orders that read 2, 5 and 7 of K's components."""
    prob, u = _case(Nt)
    e = _engine(prob, 3, monkeypatch, S=S)
    J, g = _eval_dev(e, u, order)
    e.close()
    _check(u, J, g, _oracle(Nt, order=order), (Nt, S, order))


@pytest.mark.parametrize("amp", [1.0, 8.0, 14.0])
def test_pauli_series_degree_classes(built_lib, monkeypatch, amp):
    """The series classes K = 5, 7, 9 (tests/test_gpu_blkseg_su2.py): each has its own instance of the two loops."""
    prob, u = _case(40, amp)
    e = _engine(prob, 3, monkeypatch)
    J, g = _eval_dev(e, u)
    e.close()
    _check(u, J, g, _oracle(40, amp), (amp,))


def test_pauli_one_long_segment(built_lib, monkeypatch):
    """Nt = 400 in one segment (the cap allows S = 1), B = 1: 400 rotations of one Ĝ in a row, the recursion's drift
    on the device at the same bars."""
    prob, u = _case(400)
    e = _engine(prob, 1, monkeypatch, S=1)
    J, g = _eval_dev(e, u[:1])
    e.close()
    J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[0], prob.x0, prob.x_target, prob.n, order=3)
    _assert_seed(J[0], g[0], J0, g0, ("long",))


def test_pauli_split_form_bitwise(built_lib, monkeypatch):
    """propagate_device + grape_sensitivity_device (G through HBM, turned by z̄ and taken to its Pauli components by the
    backward launch) bitwise the fused eval, at order 3, Nt = 37 in 7 segments."""
    prob, u = _case(37)
    e = _engine(prob, 3, monkeypatch, S=7)
    J, g = split_dev(e, u, 3)
    info = e.info()
    assert info["split_forward"] == "segmented" and info["backward"] == "segmented", info
    Jf, gf = _eval_dev(e, u, 3)
    e.close()
    assert np.array_equal(J, Jf) and np.array_equal(g, gf)
    _check(u, J, g, _oracle(37), ("split",))


def test_pauli_outside_the_class(built_lib, monkeypatch):
    """One control with a nonzero diagonal entry (tests/test_gpu_blkseg_su2.py::test_su2_neighbouring_classes): not
    zero-diagonal, so the general 2-row form runs on the matrix G and still matches the oracle."""
    prob, u = _case(37)
    D = np.zeros(prob.N)
    D[3] = 0.04
    prob = dataclasses.replace(prob, A=[prob.A[0] + 1j * np.diag(D), prob.A[1]])
    for M in [prob.A0] + list(prob.A):
        assert np.array_equal(M, -M.conj().T)
    e = _engine(prob, 3, monkeypatch, S=7)
    J, g = _eval_dev(e, u)
    e.close()
    for b in range(3):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3)
        _assert_seed(J[b], g[b], J0, g0, ("control_diagonal", b))
