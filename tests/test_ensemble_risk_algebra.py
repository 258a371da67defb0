"""CPU: the risk measures over a generator ensemble (qoc_amd/robust.py; include/qoc.h qoc_set_ensemble_objective) on
numpy and the oracle alone.  ensemble_risk is the reference of tests/test_gpu_ensemble_risk.py; here its own algebra:
the weights sum to W, the limits, the cancellation-free soft-max, ties, exact zeros, the NaN rule, active_bound, and
Σ_e ω_e dJ_e/du against a central difference of J̄.
"""
import numpy as np
import pytest

from qoc_amd.robust import active_bound, ensemble_risk
from risk_util import RANK_W, assert_conditions, ens_case, reference, weights
from ensemble_util import ensemble_eval

EPS = np.finfo(np.float64).eps
KINDS = [("mean", None), ("max", None), ("cvar", 0.25), ("cvar", 0.4), ("cvar", 1.0), ("lse", 1e-6), ("lse", 20.0),
         ("lse", 1e4)]


@pytest.mark.parametrize("kind,param", KINDS)
def test_weights_are_nonnegative_and_sum_to_W(kind, param):
    rng = np.random.default_rng(11)
    w = np.array([0.3, 0.0, 0.45, 0.15, 0.6])
    Jm = rng.uniform(0.1, 0.9, size=(7, 5))
    Jb, om = ensemble_risk(Jm, w, kind, param)
    assert Jb.shape == (7,) and om.shape == (7, 5)
    assert (om >= 0).all() and np.abs(om.sum(axis=1) - w.sum()).max() <= 8 * EPS * w.sum()
    assert (om[:, 1] == 0).all()  # a member without weight never carries any
    # J̄ lies between the mean and the maximum over the members with weight
    mean = Jm @ w
    mx = w.sum() * Jm[:, w > 0].max(axis=1)
    assert (Jb >= mean - 1e-14).all() and (Jb <= mx + 1e-14).all()


def test_limits():
    rng = np.random.default_rng(12)
    w = np.array([0.5, 0.3, 0.2])
    # costs within a range R = 0.05: the soft-max exceeds the mean by at most W β R² / 8 (Hoeffding's lemma), 3e-13 at
    # β = 1e-9, so the 1e-12 below is a statement about rounding and not about β
    Jm = 0.3 + 0.05 * rng.uniform(size=(5, 3))
    mean = Jm @ w
    mx = w.sum() * Jm.max(axis=1)
    assert np.abs(ensemble_risk(Jm, w, "cvar", 1.0)[0] - mean).max() <= 1e-12
    assert np.abs(ensemble_risk(Jm, w, "lse", 1e-9)[0] - mean).max() <= 1e-12
    assert np.abs(ensemble_risk(Jm, w, "cvar", 1.0)[1] - w).max() <= 1e-12
    Jx, ox = ensemble_risk(Jm, w, "max")
    assert np.array_equal(Jx, mx)
    Jb, om = ensemble_risk(Jm, w, "cvar", 0.05)  # α below every member's share
    assert np.abs(Jb - mx).max() <= 1e-12 and np.abs(om - ox).max() <= 1e-12
    # β = 1e6, β (gap) >> 1: the weights are the maximum's, and W M - J̄ lies in [0, W log(W / min w) / β]
    # (s >= w_{e*} / W - 1: the worst member's own term)
    Jb, om = ensemble_risk(Jm, w, "lse", 1e6)
    top = np.sort(Jm, axis=1)
    assert (1e6 * (top[:, -1] - top[:, -2]) > 40).all()  # e^-40 < 1e-12: the cases do test the limit
    assert np.abs(om - ox).max() <= 1e-12
    assert (mx - Jb >= -1e-15).all() and (mx - Jb <= w.sum() * np.log(w.sum() / w.min()) / 1e6 + 1e-15).all()
    # a member without weight does not enter the maximum
    J0, o0 = ensemble_risk([0.9, 0.2, 0.5], [0.0, 0.5, 0.5], "max")
    assert J0 == 0.5 and np.array_equal(o0, [0.0, 0.0, 1.0])


def test_soft_max_at_small_beta_needs_the_expm1_form():
    """Costs with a spread of 1e-3 at β = 1e-6: the expm1 / log1p form agrees with a numpy.longdouble evaluation to
    1e-15 W; the plain log Σ exp form loses ε / β ≈ 2e-10 to cancellation and does not."""
    assert np.finfo(np.longdouble).eps < EPS  # (the x87 extended format: the truth below is wider than the code under test)
    rng = np.random.default_rng(13)
    w = np.array([0.5, 0.3, 0.2, 0.4])
    W = w.sum()
    beta = 1e-6
    worst_plain = 0.0
    for _ in range(20):
        J = 0.3 + 1e-3 * rng.uniform(size=4)
        Jb, _ = ensemble_risk(J, w, "lse", beta)
        Jl, wl, bl = J.astype(np.longdouble), w.astype(np.longdouble), np.longdouble(beta)
        Wl = wl.sum()
        Ml = Jl.max()
        truth = Wl * (Ml + np.log1p(np.sum(wl / Wl * np.expm1(bl * (Jl - Ml)))) / bl)
        assert abs(np.longdouble(Jb) - truth) <= 1e-15 * W, float(np.longdouble(Jb) - truth)
        plain = W * np.log(np.sum(w / W * np.exp(beta * J))) / beta
        worst_plain = max(worst_plain, abs(float(np.longdouble(plain) - truth)))
    print("plain log-sum-exp error", worst_plain)
    assert worst_plain > 1e-15 * W


def test_ties_go_to_the_lowest_member():
    w = np.array([0.25, 0.25, 0.5])
    J = np.array([0.4, 0.7, 0.7])
    assert np.array_equal(ensemble_risk(J, w, "max")[1], [0.0, 1.0, 0.0])
    Jb, om = ensemble_risk(J, w, "cvar", 0.25)  # member 1 fills the whole α W
    assert np.array_equal(om, [0.0, 1.0, 0.0]) and Jb == 0.7
    Jb, om = ensemble_risk(J, w, "cvar", 0.5)   # member 1 first, then half of α W from member 2
    assert np.array_equal(om, [0.0, 0.5, 0.5]) and Jb == 0.7
    assert np.array_equal(ensemble_risk([0.3, 0.3], [0.5, 0.5], "cvar", 0.5)[1], [1.0, 0.0])
    assert np.array_equal(ensemble_risk([0.3, 0.3], [0.5, 0.5], "lse", 20.0)[1], [0.5, 0.5])
    assert ensemble_risk([0.3, 0.3], [0.5, 0.5], "lse", 20.0)[0] == 0.3


def test_exact_zeros_on_rank():
    """"rank" at α = 0.25: the worst member of pulses 1 and 2 is 3 (w = 0.25 = α W: it takes everything); pulse 0's
    worst is 2 (w = 0.125), then 3 fills the other half."""
    Jm, _ = reference("rank")
    w = weights("rank")
    assert [int(j.argmax()) for j in Jm] == [2, 3, 3, 2, 2, 2]
    assert len({tuple(np.argsort(-j)) for j in Jm}) > 1  # the descending orders differ between pulses
    assert_conditions(Jm, w, "cvar", 0.25)
    _, om = ensemble_risk(Jm, w, "cvar", 0.25)
    assert np.array_equal(om[1], [0, 0, 0, 1, 0]) and np.array_equal(om[2], [0, 0, 0, 1, 0])
    assert om[0][2] == 0.5 and om[0][3] == 0.5 and om[0][[0, 1, 4]].tolist() == [0, 0, 0]


def test_nan_rule():
    w = np.array(RANK_W)
    Jm = np.array([[0.1, 0.2, np.nan, 0.4, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5], [0.1, np.inf, 0.3, 0.4, 0.5]])
    for kind, param in KINDS[1:]:
        Jb, om = ensemble_risk(Jm, w, kind, param)
        assert np.isnan(om[0]).all() and np.isnan(Jb[0]) and np.isnan(om[2]).all() and np.isnan(Jb[2])
        assert np.isfinite(om[1]).all() and np.isfinite(Jb[1])
    # a non-finite cost of a member without weight is not looked at
    Jb, om = ensemble_risk([np.nan, 0.2, 0.3], [0.0, 0.5, 0.5], "max")
    assert Jb == 0.3 and np.array_equal(om, [0.0, 0.0, 1.0])


def test_active_bound():
    assert active_bound(RANK_W, 0.25) == 2
    assert active_bound(RANK_W, 0.125) == 1
    assert active_bound(RANK_W, 1.0) == 5
    assert active_bound([0.5, 0.0, 0.5], 1.0) == 2
    # a bound indeed: no costs give more active members
    rng = np.random.default_rng(14)
    for alpha in (0.1, 0.25, 0.4, 0.7):
        n = active_bound(RANK_W, alpha)
        for _ in range(50):
            om = ensemble_risk(rng.uniform(size=5), RANK_W, "cvar", alpha)[1]
            assert np.count_nonzero(om) <= n
    with pytest.raises(ValueError):
        active_bound(RANK_W, 0.0)
    with pytest.raises(ValueError):
        ensemble_risk([0.1, 0.2], [0.5, 0.5], "cvar", 1.5)
    with pytest.raises(ValueError):
        ensemble_risk([0.1, 0.2], [0.5, 0.5], "lse", np.inf)
    with pytest.raises(ValueError):
        ensemble_risk([0.1, 0.2], [0.5, 0.5], "median")


@pytest.mark.parametrize("kind,param", [("lse", 20.0), ("cvar", 0.4)])
@pytest.mark.parametrize("name", ["tiny", "rank"])
def test_weighted_member_gradients_are_the_derivative_of_the_risk(name, kind, param):
    """Σ_e ω_e g_e · d against (J̄(u + h d) - J̄(u - h d)) / 2h along a random direction, the oracle in exact mode, pulse
    0: relative 1e-6, the bar tests/test_oracle.py uses for finite differences."""
    prob, u, A0s, As, _, _ = ens_case(name)
    w = weights(name)
    u = u[0]

    def Jbar(v):
        return ensemble_risk(ensemble_eval(prob, v, A0s, As, w, order="exact")[0], w, kind, param)[0]
    Jm, gm, _, _ = ensemble_eval(prob, u, A0s, As, w, order="exact")
    assert_conditions(Jm, w, kind, param)
    _, om = ensemble_risk(Jm, w, kind, param)
    d = np.random.default_rng(15).standard_normal(u.shape)
    h = 1e-5
    fd = (Jbar(u + h * d) - Jbar(u - h * d)) / (2 * h)
    an = float(np.sum(np.tensordot(om, gm, axes=1) * d))
    print(name, kind, "fd", fd, "analytic", an)
    assert abs(fd - an) <= 1e-6 * abs(an)
