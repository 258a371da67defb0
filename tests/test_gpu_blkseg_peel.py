"""The peeled slice loops of the segmented block eval (csrc/qoc_blkseg.hpp, loop1z / loop3z): the steps below Lf, the
last segment's length, run in loops of their own without selects; the steps at and above Lf run with them (phase 3:
first, phase 1: last, pairs cut by an odd Lf or an odd L included).  Shapes through QOC_BLKSEG_S on the cavity with 10
blocks of 2 rows that hit every boundary of the two loops:

    Nt  S   L  Lf
    48  6   8   8   the select loop runs zero times
    43  6   8   3   an odd Lf cuts a pair of phase 1
    41  6   7   6   odd L: the last pair is half past the end
     9  8   2   1   S trimmed to 5
     7  7   1   1   L = 1
     1  -   1   1   a single slice

each at the three series classes of the closed form (K = 5, 7, 9), at an amplitude with a halving (the generic loops),
and at orders 1, 3 and exact; one shape of each Lf kind also with the guard-state penalty, on random permuted blocks of
3 rows and in the split form (bitwise the fused one).  Against oracle/qoc_oracle.grape_eval at the bars of
tests/blkseg_util.py: |ΔJ| <= 1e-12 and ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed.  tools/blkseg_bits.py runs the same
cases for a bitwise comparison of two builds of the library.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import assert_seed, block_problem, case, engine, eval_dev, pen, split_dev

pytestmark = pytest.mark.gpu

B = 3
# (Nt, QOC_BLKSEG_S, L, Lf)
SHAPES = [(48, 6, 8, 8), (43, 6, 8, 3), (41, 6, 7, 6), (9, 8, 2, 1), (7, 7, 1, 1), (1, None, 1, 1)]
LF_KINDS = [(48, 6), (43, 6), (41, 6)]  # Lf = L, odd Lf < L, odd L
# ρ = 0.154 + 0.05 amp at the full amplitude (tests/test_gpu_blkseg.py::test_segmented_series_degree_classes):
# K = 5 up to 0.24, 7 up to 0.66, 9 up to θ_cap ≈ 0.98, halvings beyond
AMPS = {5: 1.0, 7: 8.0, 9: 14.0, "halving": 22.0}
RHO_ABOVE = {5: 0.0, 7: 0.24, 9: 0.66, "halving": 0.98}


def seg_shape(Nt, S, nblk=10, W=8):
    """(S, L, Lf) as qoc_run_blkseg.hip's blkseg_shape derives them (one seed per CU: 8 waves of 64 / nblk segments)."""
    S0 = max(1, min(W * (64 // nblk), Nt))
    if S is not None:
        S0 = max(1, min(S0, S))
    L = -(-Nt // S0)
    S1 = -(-Nt // L)
    return S1, L, Nt - (S1 - 1) * L


@functools.lru_cache(maxsize=None)
def cavity(Nt, cls=5):
    """The cavity problem and controls of B seeds scaled as the series-class tests scale them; one slice per seed is
    set to the full amplitude, so that the seed's largest ρ_k is in the class's range whatever Nt is."""
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=Nt)  # N = 20, 10 blocks of 2, m = 2
    amp = AMPS[cls]
    u = systems.cavity_controls(B, Nt, seed=900 + Nt) * amp
    for b in range(B):
        u[b, :, (7 * b + 3) % Nt] = (0.05 * amp, -0.05 * amp)
    rad = []
    for A in [p.A0] + list(p.A):  # spectral half-widths: a lower bound of the kernel's ρ
        ev = np.linalg.eigvalsh(1j * np.asarray(A))
        rad.append(0.5 * (ev[-1] - ev[0]))
    for b in range(B):
        rho = max(rad[0] + sum(abs(u[b, j, k]) * rad[j + 1] for j in range(2)) for k in range(Nt))
        assert rho > RHO_ABOVE[cls], (cls, b, rho)
    u.setflags(write=False)
    return p, u


@functools.lru_cache(maxsize=None)
def oracle(Nt, cls=5, order=3, penalised=False):
    """The oracle's (J, dJdu) of every seed: computed once, shared, never changed."""
    p, u = cavity(Nt, cls)
    penalty = pen(case("cavity20")[2]) if penalised else None
    return tuple(O.grape_eval(p.A0, p.A, u[b], p.x0, p.x_target, p.n, order=order, penalty=penalty)[:2]
                 for b in range(B))


@functools.lru_cache(maxsize=None)
def blocks3(Nt):
    p, u, _ = block_problem(3, 3, 2, 2, Nt, seed=930 + Nt)
    ref = tuple(O.grape_eval(p.A0, p.A, u[b], p.x0, p.x_target, p.n, order=3)[:2] for b in range(u.shape[0]))
    return p, u, ref


def fused(e, u, order=3):
    out = eval_dev(e, u, order)
    assert e.info()["backward"] == "segmented", e.info()
    return out


def split(e, u, order=3):
    out = split_dev(e, u, order)
    info = e.info()
    assert info["split_forward"] == "segmented" and info["backward"] == "segmented", info
    return out


def check(J, g, ref, tag):
    for b in range(len(ref)):
        assert_seed(J[b], g[b], ref[b][0], ref[b][1], tag + (b,))


def test_shape_table():
    """The table of the module's docstring is what the host derives from Nt and QOC_BLKSEG_S."""
    for Nt, S, L, Lf in SHAPES:
        assert seg_shape(Nt, S)[1:] == (L, Lf), (Nt, S, seg_shape(Nt, S))
    assert seg_shape(9, 8)[0] == 5


@pytest.mark.parametrize("cls", [5, 7, 9, "halving"])
@pytest.mark.parametrize("Nt,S,L,Lf", SHAPES)
def test_peel_series_classes_and_halving(built_lib, monkeypatch, Nt, S, L, Lf, cls):
    """Order 3 at K = 5, 7, 9 (the peeled fast loops, one instance per class) and beyond θ_cap (the generic loops)."""
    p, u = cavity(Nt, cls)
    e = engine(p, B, monkeypatch, S=S)
    J, g = fused(e, u)
    e.close()
    check(J, g, oracle(Nt, cls), (Nt, S, cls))


@pytest.mark.parametrize("order", [1, "exact"])
@pytest.mark.parametrize("Nt,S,L,Lf", SHAPES)
def test_peel_orders(built_lib, monkeypatch, Nt, S, L, Lf, order):
    """Orders 1 and exact (order 3: above) on every shape."""
    p, u = cavity(Nt)
    e = engine(p, B, monkeypatch, S=S)
    J, g = fused(e, u, order)
    e.close()
    check(J, g, oracle(Nt, order=order), (Nt, S, order))


@pytest.mark.parametrize("order", [1, 3, "exact"])
@pytest.mark.parametrize("Nt,S", LF_KINDS)
def test_peel_split_form_bitwise(built_lib, monkeypatch, Nt, S, order):
    """propagate_device + grape_sensitivity_device (the backward launch runs phase 3's two loops alone) bitwise the
    fused eval."""
    p, u = cavity(Nt)
    e = engine(p, B, monkeypatch, S=S)
    Js, gs = split(e, u, order)
    J, g = fused(e, u, order)
    e.close()
    assert np.array_equal(J, Js) and np.array_equal(g, gs)
    check(J, g, oracle(Nt, order=order), ("split", Nt, S, order))


@pytest.mark.parametrize("Nt,S", LF_KINDS)
def test_peel_penalised(built_lib, monkeypatch, Nt, S):
    """With the guard-state penalty of tests/blkseg_util.py's cavity20 case (H in phase 1, D and the source in phase
    3, in both variants of a step): against the oracle's penalised values, fused and split bitwise equal."""
    p, u = cavity(Nt)
    e = engine(p, B, monkeypatch, pen=pen(case("cavity20")[2]), S=S)
    J, g = fused(e, u)
    Js, gs = split(e, u)
    e.close()
    assert np.array_equal(J, Js) and np.array_equal(g, gs)
    check(J, g, oracle(Nt, penalised=True), ("pen", Nt, S))


@pytest.mark.parametrize("Nt,S", LF_KINDS)
def test_peel_blocks_of_3_rows(built_lib, monkeypatch, Nt, S):
    """Random permuted blocks of 3 rows with a padded one (the generic loops, which share the scaffolding), fused and
    split bitwise equal."""
    p, u, ref = blocks3(Nt)
    e = engine(p, u.shape[0], monkeypatch, S=S)
    J, g = fused(e, u)
    Js, gs = split(e, u)
    e.close()
    assert np.array_equal(J, Js) and np.array_equal(g, gs)
    check(J, g, ref, ("blocks3", Nt, S))
