"""CPU: the algebra behind the generator ensemble (include/qoc.h qoc_set_generator_ensemble) on the oracle alone.

The reference of the GPU tests (tests/ensemble_util.py) is Σ_e w_e qoc_oracle.grape_eval(member e); here its gradient is
held against a central difference of J̄ itself, and systems.ensemble_members against what the engine's setter demands of
every member: exactly skew-Hermitian generators (the test qoc_set_generators applies) whose off-diagonal entries stay
inside the invariant blocks of the nominal set.
"""
import numpy as np
import pytest

from ensemble_util import CASES, ens_case, ensemble_eval, weights


def test_ensemble_gradient_is_the_derivative_of_the_weighted_cost():
    """dJ̄/du of the helper in exact mode against (J̄(u + h d) - J̄(u - h d)) / 2h along a random direction: relative
    1e-6, the bar tests/test_oracle.py uses for finite differences."""
    prob, u, A0s, As, _, _ = ens_case("tiny")
    w = weights("tiny")
    u = u[0]
    Jm, gm, Jbar, gbar = ensemble_eval(prob, u, A0s, As, w, order="exact")
    assert Jbar == float(Jm @ w) and np.array_equal(gbar, np.tensordot(w, gm, axes=1))
    d = np.random.default_rng(7).standard_normal(u.shape)
    h = 1e-5
    fd = (ensemble_eval(prob, u + h * d, A0s, As, w, order="exact")[2]
          - ensemble_eval(prob, u - h * d, A0s, As, w, order="exact")[2]) / (2 * h)
    an = float(np.sum(gbar * d))
    print("fd", fd, "analytic", an)
    assert abs(fd - an) <= 1e-6 * abs(an)
    # and the members do differ: a reference that ignored the members would not see it
    assert np.ptp(Jm) > 1e-6


def _blocks(gens):
    """Connected components of the union sparsity pattern (the engine's blk_detect): block id per row."""
    N = gens[0].shape[0]
    par = list(range(N))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x
    for G in gens:
        for r, c in zip(*np.nonzero(G)):
            if r != c:
                a, b = find(r), find(c)
                par[max(a, b)] = min(a, b)
    return np.array([find(r) for r in range(N)])


@pytest.mark.parametrize("name", CASES)
def test_members_stay_skew_hermitian_and_inside_the_nominal_blocks(name):
    prob, _, A0s, As, _, _ = ens_case(name)
    blk = _blocks([prob.A0] + list(prob.A))
    assert np.bincount(blk).max() in (2, 3)
    eps = np.finfo(np.float64).eps
    for e in range(A0s.shape[0]):
        for G in [A0s[e]] + [a[e] for a in As]:
            assert np.abs(G + G.conj().T).max() <= 4 * eps * np.abs(G).max()  # the engine's exact test
            r, c = np.nonzero(G)
            off = r != c
            assert np.array_equal(blk[r[off]], blk[c[off]])
    # the members are not copies of one another
    assert A0s.shape[0] == 1 or any(not np.array_equal(A0s[0], A0s[e]) or not np.array_equal(As[0][0], As[0][e])
                                    for e in range(1, A0s.shape[0]))


def test_ensemble_members_arguments():
    from qoc_amd import systems
    prob = ens_case("tiny")[0]
    A0s, As = systems.ensemble_members(prob, amp_scales=(1.0, 0.5))
    assert A0s.shape == (2, prob.N, prob.N) and len(As) == prob.nu
    assert np.array_equal(A0s[1], prob.A0) and np.array_equal(As[1][1], prob.A[1] * 0.5)
    A0s, As = systems.ensemble_members(prob, dA0=[prob.A0 * 0.1])
    assert np.array_equal(A0s[0], prob.A0 + prob.A0 * 0.1) and np.array_equal(As[0][0], prob.A[0])
    with pytest.raises(ValueError):
        systems.ensemble_members(prob)
    with pytest.raises(ValueError):
        systems.ensemble_members(prob, dA0=[prob.A0], amp_scales=(1.0, 2.0))
    with pytest.raises(ValueError):
        systems.ensemble_members(prob, dA0=[np.zeros((2, 2))])
