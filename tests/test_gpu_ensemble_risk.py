"""GPU: worst-case, CVaR and soft-max objectives over a generator ensemble (include/qoc.h qoc_set_ensemble_objective;
k_ens_weights, k_ens_reduce_w and the ENS instantiations of the segmented eval's halves, csrc/qoc_blkseg.hpp).

The reference is tests/risk_util.py: member costs and gradients from the oracle, J̄ and ω from
qoc_amd.robust.ensemble_risk; its docstring has the bars and the conditions asserted on the reference.  Route 1 is the
fused launch for every (pulse, member), route 2 the forward half for all and the backward half where ω is not 0;
QOC_ENS_SKIP=0|1 forces one when a setter derives it.  Every test needs the new entry points.
"""
import numpy as np
import pytest

from blkseg_util import bufs, dev, engine
from ensemble_util import zcal_family_match
from risk_util import EPS, assert_conditions, assert_risk, ens_case, reference, weights

pytestmark = pytest.mark.gpu

EX = "exact"
ALPHA = {"rank": 0.4, "cavity": 0.4, "zz": 0.5, "mixed": 0.4, "cavity20_pen": 0.5, "many": 0.3}


def _set(e, name):
    _, _, A0s, As, w, _ = ens_case(name)
    e.set_generator_ensemble(A0s, As, w)


def _objective(e, monkeypatch, kind, param=None, skip=None):
    """set_ensemble_objective with QOC_ENS_SKIP set (0 / 1) or cleared (None) while the route is derived."""
    if skip is None:
        monkeypatch.delenv("QOC_ENS_SKIP", raising=False)
    else:
        monkeypatch.setenv("QOC_ENS_SKIP", str(skip))
    e.set_ensemble_objective(kind, param)


def _eval(e, u, order=3):
    """eval_device on fresh NaN-filled buffers -> J̄ (B,), dJ̄/du (B, nu, Nt), member costs and ω (B, E)."""
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), e.member_costs(), e.member_weights()


def _both_routes(e, monkeypatch, u, order, kind, param):
    """The same eval under QOC_ENS_SKIP=1 and =0: the same J̄, ω and dJ̄/du bit for bit, reported as route 2 and 1."""
    _objective(e, monkeypatch, kind, param, skip=1)
    r2 = _eval(e, u, order)
    assert e.ensemble_objective == (kind, param, 2)
    _objective(e, monkeypatch, kind, param, skip=0)
    r1 = _eval(e, u, order)
    assert e.ensemble_objective == (kind, param, 1)
    for a, b in zip(r2, r1):
        assert np.array_equal(a, b)
    return r2


@pytest.mark.parametrize("kind,param", [("mean", None), ("max", None), ("cvar", 0.25), ("cvar", 0.4), ("cvar", 1.0),
                                        ("lse", 1e-6), ("lse", 20.0), ("lse", 1e4)])
def test_rank_every_objective(built_lib, monkeypatch, kind, param):
    """"rank" (3 blocks of 2 rows, Nt = 16, B = 6, E = 5, dyadic weights; the pulses' worst members and orders differ)
    under every objective, on the route the engine chooses.  At α = 0.25 the weights are the exact zeros and halves of
    tests/test_ensemble_risk_algebra.py; at β = 1e4 some ω underflow to exactly 0 and are skipped."""
    prob, u, *_ = ens_case("rank")
    w = weights("rank")
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "rank")
    _objective(e, monkeypatch, kind, param)
    assert e.ensemble_objective == (kind, param, 0)
    J, g, Jm, om = _eval(e, u)
    assert e.ensemble_objective[2] in (1, 2)
    assert_risk(J, g, Jm, om, reference("rank"), range(u.shape[0]), w, kind, param, ("rank", kind, param))
    assert np.isfinite(g).all()
    if kind == "mean":
        assert np.array_equal(om, np.tile(w, (u.shape[0], 1))) and e.member_weights_device() == 0
    else:
        assert e.member_weights_device() != 0
    if (kind, param) == ("cvar", 0.25):
        assert np.array_equal(om[1], [0, 0, 0, 1, 0]) and np.array_equal(om[2], [0, 0, 0, 1, 0])
        assert np.array_equal(om[0], [0, 0, 0.5, 0.5, 0])
    if (kind, param) == ("lse", 1e4):
        assert (om == 0).any()
    e.close()


@pytest.mark.parametrize("kind", ["max", "cvar"])
@pytest.mark.parametrize("order", [3, EX])
@pytest.mark.parametrize("name", ["cavity", "zz"])
def test_both_routes(built_lib, monkeypatch, name, order, kind):
    """cavity (blocks of 2 rows, Nt = 37: segment tails) and zz (blocks of 3 rows), E = 3, under the trace cost: route 2
    and route 1 give the same bits, and those meet the bars."""
    prob, u, *_ = ens_case(name)
    w = weights(name)
    param = ALPHA[name] if kind == "cvar" else None
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, name)
    J, g, Jm, om = _both_routes(e, monkeypatch, u, order, kind, param)
    assert_risk(J, g, Jm, om, reference(name, order), range(u.shape[0]), w, kind, param, (name, order, kind))
    e.close()


@pytest.mark.parametrize("kind", ["max", "cvar"])
@pytest.mark.parametrize("order", [3, EX])
def test_both_routes_zcal(built_lib, monkeypatch, order, kind):
    """zz under the z-calibrated cost.  J̄ and ω to the bars; the gradient carries each member's calibration phase,
    which two correct searches fix only to ~sqrt(eps) (ensemble_util's docstring): it is held against the family
    Σ_e ω_e g_e(Δθ_e) with the engine's ω, to the same residual 1e-10."""
    from ensemble_util import reference as zref
    from qoc_amd.robust import ensemble_risk
    prob, u, A0s, As, _, _ = ens_case("zz")
    w = weights("zz")
    param = ALPHA["zz"] if kind == "cvar" else None
    e = engine(prob, u.shape[0], monkeypatch)
    e.set_cost_zcalibrated(prob.x_target)
    _set(e, "zz")
    J, g, Jm, om = _both_routes(e, monkeypatch, u, order, kind, param)
    Jmr = zref("zz", order, True)[0]
    assert_conditions(Jmr, w, kind, param)
    for b in range(u.shape[0]):
        Jr, omr = ensemble_risk(Jmr[b], w, kind, param)
        res, dth = zcal_family_match(g[b], prob, u[b], A0s, As, om[b], order)
        print(("zz zcal", order, kind, b), "dJbar", J[b] - Jr, "d omega", np.abs(om[b] - omr).max(), "residual", res)
        assert np.abs(Jm[b] - Jmr[b]).max() <= 1e-12 and abs(J[b] - Jr) <= 1e-12 * w.sum()
        assert np.abs(om[b] - omr).max() <= 32 * EPS * w.sum()
        assert res <= 1e-10, (order, kind, b, res)
    e.close()


@pytest.mark.parametrize("order", [3, EX])
def test_mixed_kernel_classes_on_route_2(built_lib, monkeypatch, order):
    """Three kernel classes in one launch (zero-diagonal SU(2) loops | the general 2-row form | halvings and the generic
    exact series) through the forward and the member-aware backward half."""
    prob, u, *_ = ens_case("mixed")
    w = weights("mixed")
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "mixed")
    for kind, param in (("max", None), ("cvar", ALPHA["mixed"])):
        _objective(e, monkeypatch, kind, param, skip=1)
        J, g, Jm, om = _eval(e, u, order)
        assert e.ensemble_objective[2] == 2
        assert_risk(J, g, Jm, om, reference("mixed", order), range(u.shape[0]), w, kind, param, ("mixed", order, kind))
    e.close()


def test_penalised_backward_half(built_lib, monkeypatch):
    """cavity20 with its guard-state penalty, E = 2, the worst member on route 2: the penalised forward half writes D
    beside G per (pulse, member), the penalised backward half reads them."""
    prob, u, _, _, _, pn = ens_case("cavity20_pen")
    w = weights("cavity20_pen")
    e = engine(prob, u.shape[0], monkeypatch, pen=pn)
    _set(e, "cavity20_pen")
    for order in (3, EX):
        J, g, Jm, om = _both_routes(e, monkeypatch, u, order, "max", None)
        assert_risk(J, g, Jm, om, reference("cavity20_pen", order), range(u.shape[0]), w, "max", None,
                    ("cavity20_pen", order))
    e.close()


def test_more_workgroups_than_compute_units(built_lib, monkeypatch):
    """B = 40, E = 7 (280 workgroups, random weights) with CVaR: parity on pulses 0, 17 and 39, and every pulse's ω is
    ensemble_risk of its own member costs."""
    from qoc_amd.robust import ensemble_risk
    prob, u, *_ = ens_case("many")
    w = weights("many")
    a = ALPHA["many"]
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "many")
    J, g, Jm, om = _both_routes(e, monkeypatch, u, 3, "cvar", a)
    assert_risk(J, g, Jm, om, reference("many", 3, (0, 17, 39)), (0, 17, 39), w, "cvar", a, ("many",))
    Jo, oo = ensemble_risk(Jm, w, "cvar", a)
    assert np.abs(om - oo).max() <= 32 * EPS * w.sum() and np.abs(J - Jo).max() <= 32 * EPS * w.sum()
    assert np.isfinite(g).all()
    e.close()


def test_the_skip_is_real(built_lib, monkeypatch):
    """The member gradients filled with NaN before a route-2 eval of "rank" under MAX: dJ̄/du is finite, each pulse's
    worst member's row is finite, and the other four rows are still all NaN (their workgroups wrote nothing, and the
    reduction did not read them)."""
    import torch
    from qoc_amd.optimize import _DevView
    prob, u, *_ = ens_case("rank")
    B, nu, Nt = u.shape
    E = 5
    e = engine(prob, B, monkeypatch)
    _set(e, "rank")
    _objective(e, monkeypatch, "max", skip=1)
    gm = torch.as_tensor(_DevView(e.member_grads_device(), (B * E, Nt * nu), "<f8"), device=torch.device("cuda", 0))
    e.synchronize()
    gm.fill_(float("nan"))
    torch.cuda.synchronize()
    J, g, Jm, om = _eval(e, u)
    assert e.ensemble_objective[2] == 2
    rows = gm.cpu().numpy().reshape(B, E, Nt * nu)
    assert np.isfinite(g).all() and np.isfinite(J).all()
    for b in range(B):
        worst = int(Jm[b].argmax())
        assert om[b][worst] == 1.0 and np.count_nonzero(om[b]) == 1
        assert np.isfinite(rows[b, worst]).all()
        assert np.isnan(np.delete(rows[b], worst, axis=0)).all()
    e.close()


@pytest.mark.parametrize("order", [3, EX])
def test_bitwise_ties(built_lib, monkeypatch, order):
    """With the launch shape pinned (QOC_BLKSEG_W, QOC_BLKSEG_S): two copies of the nominal set with weights (0.5, 0.5)
    give the plain eval's J and dJdu bit for bit under MAX, CVaR α = 0.5 and LSE β = 20, with ω = (1, 0), (1, 0) and
    (0.5, 0.5); back under "mean" the eval is bitwise the one before any objective was set; after clearing the ensemble
    the plain eval is bitwise the plain eval."""
    from qoc_amd import systems
    prob = ens_case("cavity")[0]
    u5 = systems.cavity_controls(5, prob.Nt, seed=96)
    e = engine(prob, 5, monkeypatch, W=2, S=16)
    J0, g0, _, _ = _eval_plain(e, u5, order)
    nom = np.stack([prob.A0, prob.A0]), [np.stack([a, a]) for a in prob.A]
    e.set_generator_ensemble(*nom, (0.5, 0.5))
    Jn, gn, _, _ = _eval(e, u5, order)
    assert np.array_equal(Jn, J0) and np.array_equal(gn, g0)
    for kind, param, want in (("max", None, (1.0, 0.0)), ("cvar", 0.5, (1.0, 0.0)), ("lse", 20.0, (0.5, 0.5))):
        for skip in (1, 0):
            _objective(e, monkeypatch, kind, param, skip=skip)
            J, g, Jm, om = _eval(e, u5, order)
            assert np.array_equal(J, J0) and np.array_equal(g, g0), (kind, skip)
            assert np.array_equal(om, np.tile(want, (5, 1))), (kind, skip, om)
            assert np.array_equal(Jm[:, 0], J0) and np.array_equal(Jm[:, 1], J0)
    _objective(e, monkeypatch, "mean")
    Jb, gb, _, omb = _eval(e, u5, order)
    assert np.array_equal(Jb, Jn) and np.array_equal(gb, gn) and np.array_equal(omb, np.full((5, 2), 0.5))
    e.clear_generator_ensemble()
    J1, g1, _, _ = _eval_plain(e, u5, order)
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    e.close()


def _eval_plain(e, u, order=3):
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), None, None


def _raises(code, f, *a, **k):
    from qoc_amd import QOCError
    with pytest.raises(QOCError) as ei:
        f(*a, **k)
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


def test_setter_contract(built_lib, monkeypatch):
    """Bad kinds and parameters: QOC_ERR_ARG and nothing changes.  The objective survives a replaced ensemble, a cleared
    one and set_generators.  member_weights() before the first eval (since a setter): QOC_ERR_STATE.  The workspace is
    counted in device_bytes and freed with the ensemble."""
    from qoc_amd import _lib
    lib = built_lib
    prob, u, A0s, As, w, _ = ens_case("cavity")
    e = engine(prob, u.shape[0], monkeypatch)
    assert e.ensemble_objective == ("mean", None, 0)
    bytes0 = e.info()["device_bytes"]
    _objective(e, monkeypatch, "cvar", 0.4)  # valid without an ensemble; nothing to allocate
    assert e.ensemble_objective == ("cvar", 0.4, 0) and e.info()["device_bytes"] == bytes0
    assert e.member_grads_device() == 0 and e.member_weights_device() == 0
    arg = _lib.QOC_ERR_ARG
    for kind, param in ((7, 0.0), (-1, 0.0), (_lib.QOC_ENS_CVAR, 0.0), (_lib.QOC_ENS_CVAR, 1.5), (_lib.QOC_ENS_CVAR, np.nan),
                        (_lib.QOC_ENS_LSE, 0.0), (_lib.QOC_ENS_LSE, -1.0), (_lib.QOC_ENS_LSE, np.inf),
                        (_lib.QOC_ENS_LSE, np.nan)):
        assert lib.qoc_set_ensemble_objective(e._h, kind, param) == arg, (kind, param)
        assert e.ensemble_objective == ("cvar", 0.4, 0)
    with pytest.raises(ValueError):
        e.set_ensemble_objective("median")
    with pytest.raises(ValueError):
        e.set_ensemble_objective("lse")
    _raises(_lib.QOC_ERR_STATE, e.member_weights)  # no ensemble
    # the ensemble's setter completes the pair: ω (and G for route 2) are allocated and counted
    monkeypatch.setenv("QOC_ENS_SKIP", "1")
    _set(e, "cavity")
    bytes_pair = e.info()["device_bytes"]
    assert e.member_grads_device() != 0 and e.member_weights_device() != 0
    _raises(_lib.QOC_ERR_STATE, e.member_weights)  # no eval yet
    J, g, Jm, om = _eval(e, u)
    assert e.ensemble_objective == ("cvar", 0.4, 2)
    assert_risk(J, g, Jm, om, reference("cavity"), range(u.shape[0]), weights("cavity"), "cvar", 0.4, ("pair",))
    # a replaced ensemble keeps the objective (and a new one has no eval yet)
    _set(e, "cavity")
    assert e.ensemble_objective == ("cvar", 0.4, 0) and e.info()["device_bytes"] == bytes_pair
    _raises(_lib.QOC_ERR_STATE, e.member_weights)
    J2, g2, _, om2 = _eval(e, u)
    assert np.array_equal(J2, J) and np.array_equal(g2, g) and np.array_equal(om2, om)
    # the other order of the pair: the objective's setter allocates (mean frees nothing; the buffers stay the ensemble's)
    _objective(e, monkeypatch, "mean")
    _raises(_lib.QOC_ERR_STATE, e.member_weights)  # the last eval's weights were the old objective's
    assert e.member_costs().shape == Jm.shape       # the member costs do not depend on the objective
    _objective(e, monkeypatch, "max", skip=1)
    assert e.info()["device_bytes"] == bytes_pair
    # set_generators and clearing drop the ensemble and its workspace, not the objective
    e.set_generators(prob.A0, prob.A)
    assert e.ensemble_size == 0 and e.ensemble_objective == ("max", None, 0)
    assert e.info()["device_bytes"] < bytes_pair
    bytes_plain = e.info()["device_bytes"]
    _set(e, "cavity")
    J3, g3, Jm3, om3 = _eval(e, u)
    assert_risk(J3, g3, Jm3, om3, reference("cavity"), range(u.shape[0]), weights("cavity"), "max", None, ("max",))
    e.clear_generator_ensemble()
    assert e.ensemble_objective == ("max", None, 0) and e.info()["device_bytes"] == bytes_plain
    e.close()


@pytest.mark.parametrize("kind,param", [("lse", 20.0), ("max", None)])
def test_refusals_hold_under_every_objective(built_lib, monkeypatch, kind, param):
    """Every refusal of tests/test_gpu_ensemble.py::test_refusals gives the same code under LSE and under MAX; refused
    calls write nothing; the co-states of the last plain backward stay readable; the penalised eval on blocks of 3 rows
    stays refused."""
    from qoc_amd import _lib, systems
    prob, u, A0s, As, w, _ = ens_case("cavity")
    B, nu, Nt = u.shape
    e = engine(prob, B, monkeypatch)
    J0, g0, _, _ = _eval_plain(e, u)
    _objective(e, monkeypatch, kind, param)
    bad = A0s.copy()
    bad[1][0, 1] = 1e-3
    bad[1][1, 0] = -1e-3
    _raises(_lib.QOC_ERR_ARG, e.set_generator_ensemble, bad, As, w)
    for ww in ((0.5, -0.1, 0.6), (0.5, np.nan, 0.5), (0.0, 0.0, 0.0), (np.inf, 1.0, 1.0)):
        _raises(_lib.QOC_ERR_ARG, e.set_generator_ensemble, A0s, As, ww)
    assert e.ensemble_size == 0
    J1, g1, _, _ = _eval_plain(e, u)  # the failed setters changed nothing; the objective does not touch a plain eval
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    lam = e.costate(Nt // 2, 1)
    _set(e, "cavity")
    _raises(_lib.QOC_ERR_STATE, e.state, 0)
    un = _lib.QOC_ERR_UNSUPPORTED
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    Bs = systems.spline_matrix(float(Nt), Nt, 4)
    e.set_spline_basis(Bs)
    c = np.zeros((B, 4, nu))
    par = np.tile([float(Nt), 5.0, 0.01, 0.1], (B, 1))
    _raises(un, e.propagate, u)
    _raises(un, e.grape_sensitivity, u)
    _raises(un, e.propagate_device, ud.data_ptr(), Jd.data_ptr())
    _raises(un, e.grape_sensitivity_device, ud.data_ptr(), 3, gd.data_ptr())
    _raises(un, e.propagate_spline, c)
    _raises(un, e.sensitivity_spline, c)
    _raises(un, e.propagate_envelope, "drag", par, float(Nt), 0.5)
    _raises(un, e.eval_envelope, "drag", par, float(Nt), 0.5)
    _raises(un, e.eval_envelope_device, "drag", ud.data_ptr(), 4, float(Nt), 0.5, Jd.data_ptr(), gd.data_ptr())
    e.set_costate_source(np.zeros((B, Nt + 1, prob.N, prob.m), complex))
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    _raises(un, e.eval_spline, c)
    e.set_costate_source(None)
    assert np.isnan(Jd.cpu().numpy()).all() and np.isnan(gd.cpu().numpy()).all()  # the refused calls wrote nothing
    _raises(_lib.QOC_ERR_STATE, e.member_weights)
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    _eval(e, u)
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    _raises(_lib.QOC_ERR_STATE, e.state, 0)
    e.close()
    # blocks of 3 rows with the penalty: refused under the objective as under the mean
    prob, u, A0s, As, w, pn = ens_case("zz_pen")
    e = engine(prob, u.shape[0], monkeypatch, pen=pn)
    _objective(e, monkeypatch, kind, param, skip=1)
    e.set_generator_ensemble(A0s, As, w)
    ud = dev(u)
    Jd, gd = bufs(u.shape[0], u.shape[2], u.shape[1])
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    _raises(_lib.QOC_ERR_STATE, e.member_weights)
    assert np.isnan(Jd.cpu().numpy()).all() and np.isnan(gd.cpu().numpy()).all()
    e.close()


@pytest.fixture(scope="module")
def zz_callers(built_lib):
    """zz, Nt = 60, ns = 6, B = 4, E = 3 under the trace cost: what the callers of qoc_eval_dev return under LSE β = 20
    (and the best pick under MAX)."""
    import torch
    from qoc_amd import GrapeEngine, systems
    from qoc_amd.optimize import minimize_on_device
    prob, _, A0s, As, _, _ = ens_case("zz")
    B, ns, nu = 4, 6, 2
    Bs = systems.spline_matrix(6.0, prob.Nt, ns)
    c0 = np.random.default_rng(97).uniform(-0.3, 0.3, size=(B, ns, nu))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    e.set_chain("taylor")
    w = (0.2, 0.5, 0.3)
    e.set_generator_ensemble(A0s, As, w)
    e.set_ensemble_objective("lse", 20.0)
    e.set_spline_basis(Bs)
    Js, dJdc = e.eval_spline(c0)
    u0 = np.einsum("tn,bnj->bjt", Bs, c0)
    Ju, gu, Jmu, omu = _eval(e, u0)
    res = minimize_on_device(e, Bs, torch.from_numpy(c0.transpose(0, 2, 1).reshape(B, nu * ns).copy()).cuda(),
                             lower=-0.4, upper=0.4, max_iter=5)
    cf = res.c.cpu().numpy().reshape(B, nu, ns).transpose(0, 2, 1)
    J_again = e.eval_spline(cf)[0]
    Jm_again, om_again = e.member_costs(), e.member_weights()
    e.set_ensemble_objective("max")
    Jx = e.eval_spline(c0)[0]
    best_x = e.allgather_best()
    Jmx = e.member_costs()
    e.close()
    return dict(Bs=Bs, w=np.asarray(w), Js=Js, dJdc=dJdc, Ju=Ju, gu=gu, Jmu=Jmu, omu=omu, f=res.f.cpu().numpy(),
                J_again=J_again, Jm_again=Jm_again, om_again=om_again, Jx=Jx, best_x=best_x, Jmx=Jmx)


def test_eval_spline_is_the_spline_map_of_the_risk_gradient(zz_callers):
    z = zz_callers
    assert np.abs(z["Js"] - z["Ju"]).max() <= 1e-12 * z["w"].sum()
    for b in range(4):
        ref = z["Bs"].T @ z["gu"][b].T  # ns x nu
        rel = np.linalg.norm(z["dJdc"][b] - ref) / np.linalg.norm(ref)
        print(b, "rel dJdc", rel)
        assert rel <= 1e-10


def test_device_optimiser_minimises_the_risk(zz_callers):
    from qoc_amd.robust import ensemble_risk
    z = zz_callers
    assert np.array_equal(z["f"], z["J_again"])  # f is the eval at the returned iterates, bit for bit
    assert (z["f"] < z["Js"]).all()              # every seed went down from its start
    Jo, oo = ensemble_risk(z["Jm_again"], z["w"], "lse", 20.0)
    assert np.abs(z["J_again"] - Jo).max() <= 32 * EPS * z["w"].sum()
    assert np.abs(z["om_again"] - oo).max() <= 32 * EPS * z["w"].sum()
    assert (z["J_again"] > z["Jm_again"] @ z["w"]).all()  # the soft-max, not the mean


def test_allgather_best_is_the_argmin_of_the_worst_case(zz_callers):
    z = zz_callers
    W = z["w"].sum()
    assert np.abs(z["Jx"] - W * z["Jmx"].max(axis=1)).max() <= 32 * EPS * W
    assert z["best_x"][0] == z["Jx"].min() and z["best_x"][1] == int(z["Jx"].argmin())
