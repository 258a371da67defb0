"""GPU: robust control over an ensemble of generator sets (include/qoc.h qoc_set_generator_ensemble; the ENS
instantiations of k_blkseg_eval and k_ens_reduce, csrc/qoc_blkseg.hpp).

With an ensemble set, eval_device returns J̄_b = Σ_e w_e J(u_b; member e) and its gradient from one launch with a
workgroup per (pulse, member) and one reduction launch.  The reference is tests/ensemble_util.py: the oracle called
once per (pulse, member); the bars are the fp64 bars of DESIGN.md §2 per pulse (|ΔJ̄| <= 1e-12 Σw, |ΔJ_be| <= 1e-12,
||ΔdJ̄du|| / ||dJ̄du|| <= 1e-10).  Every test here needs the new entry points, so none passes without them.
"""
import ctypes as C

import numpy as np
import pytest

from blkseg_util import bufs, dev, engine
from ensemble_util import assert_pulse, ens_case, reference, weights, zcal_family_match

pytestmark = pytest.mark.gpu

EX = "exact"


def _set(e, name):
    _, _, A0s, As, w, _ = ens_case(name)
    e.set_generator_ensemble(A0s, As, w)
    assert e.ensemble_size == A0s.shape[0]


def _eval(e, u, order=3):
    """eval_device on fresh NaN-filled buffers -> J (B,), dJdu (B, nu, Nt), member costs (B, E) or None."""
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    Jm = e.member_costs() if e.ensemble_size else None
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), Jm


def _parity(e, name, order, zcal=False, pulses=None):
    prob, u, A0s, As, _, _ = ens_case(name)
    w = weights(name)
    J, g, Jm = _eval(e, u, order)
    assert Jm.shape == (u.shape[0], A0s.shape[0])
    ref = reference(name, order, zcal, pulses)
    for i, b in enumerate(pulses or range(u.shape[0])):
        if not zcal:
            assert_pulse(J[b], g[b], Jm[b], ref, i, w, (name, order, b))
            continue
        # the z-calibrated cost: J to the bar, the gradient within the members' calibration-phase family
        assert abs(J[b] - ref[2][i]) <= 1e-12 * w.sum() and np.abs(Jm[b] - ref[0][i]).max() <= 1e-12
        res, dth = zcal_family_match(g[b], prob, u[b], A0s, As, w, order)
        print((name, order, b), "dJbar", J[b] - ref[2][i], "residual", res, "phases", dth)
        assert res <= 1e-10, (name, order, b, res)
    return J, g, Jm


@pytest.mark.parametrize("order", [1, 2, 3, 4, EX])
def test_parity_blocks_of_2(built_lib, monkeypatch, order):
    """cavity (N = 10, 5 blocks of 2, Nt = 37: segment tails), B = 3, E = 3, weights (0.5, 0.3, 0.2): qubit detunings
    0, ±2e-3 and amplitude scales 1, 0.97, 1.04; J̄, dJ̄/du and member_costs() per member."""
    prob, u, *_ = ens_case("cavity")
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "cavity")
    _, _, Jm = _parity(e, "cavity", order)
    assert np.ptp(Jm, axis=1).min() > 1e-6  # the members are told apart
    assert e.info()["device_bytes"] > 0
    e.close()


@pytest.mark.parametrize("order", [3, EX])
@pytest.mark.parametrize("zcal", [False, True], ids=["trace", "zcal"])
def test_parity_blocks_of_3(built_lib, monkeypatch, zcal, order):
    """zz (N = 9, 3 blocks of 3, Nt = 60), B = 3, E = 3, default weights 1/E: the ZZ strength and one anharmonicity
    scaled per member; the trace and the z-calibrated cost."""
    prob, u, *_ = ens_case("zz")
    e = engine(prob, u.shape[0], monkeypatch)
    if zcal:
        e.set_cost_zcalibrated(prob.x_target)
    _set(e, "zz")
    _parity(e, "zz", order, zcal)
    e.close()


@pytest.mark.parametrize("order", [3, EX])
def test_mixed_kernel_classes_in_one_launch(built_lib, monkeypatch, order):
    """One launch whose workgroups take three paths: member 0 keeps the zero-diagonal class (phase-free SU(2) loops),
    member 1 has a control generator with a diagonal part (the general 2-row form), member 2 an amplitude scale of 22,
    so that ρ > θ_cap: halvings and the generic exact series."""
    prob, u, A0s, As, _, _ = ens_case("mixed")
    # member 2's largest ρ_k is above θ_cap ≈ 0.98 for every pulse: |u| (λmax - λmin) / 2 summed over the controls
    rad = [np.ptp(np.linalg.eigvalsh(1j * a[2])) / 2 for a in As]
    assert (np.abs(u[:, 0]) * rad[0] + np.abs(u[:, 1]) * rad[1]).max(axis=1).min() > 1.0
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "mixed")
    _parity(e, "mixed", order)
    e.close()


def test_penalty_on_blocks_of_2(built_lib, monkeypatch):
    """The one-launch penalised kernel under an ensemble (cavity20's penalty of blkseg_util.case, E = 2)."""
    prob, u, _, _, _, pn = ens_case("cavity20_pen")
    e = engine(prob, u.shape[0], monkeypatch, pen=pn)
    _set(e, "cavity20_pen")
    _parity(e, "cavity20_pen", 3)
    _parity(e, "cavity20_pen", EX)
    e.close()


def test_penalty_on_blocks_of_3_is_refused(built_lib, monkeypatch):
    """zz's penalised eval is two launches with G and D per seed in HBM: QOC_ERR_UNSUPPORTED under an ensemble, the
    context as it was, and the plain eval after clearing is the plain eval before setting, bit for bit."""
    from qoc_amd import QOCError, _lib
    prob, u, _, _, _, pn = ens_case("zz_pen")
    e = engine(prob, u.shape[0], monkeypatch, pen=pn)
    J0, g0, _ = _eval(e, u)
    _set(e, "zz_pen")
    with pytest.raises(QOCError) as ei:
        _eval(e, u)
    assert ei.value.code == _lib.QOC_ERR_UNSUPPORTED
    with pytest.raises(QOCError) as ei:
        e.member_costs()
    assert ei.value.code == _lib.QOC_ERR_STATE  # no ensemble eval has run
    e.clear_generator_ensemble()
    J1, g1, _ = _eval(e, u)
    assert np.array_equal(J0, J1) and np.array_equal(g0, g1)
    assert e.info()["backward"] == "segmented"
    e.close()


@pytest.mark.parametrize("order", [3, EX])
def test_bitwise_ties(built_lib, monkeypatch, order):
    """With the launch shape pinned (QOC_BLKSEG_W, QOC_BLKSEG_S): two identical members equal to the nominal set with
    weights (0.5, 0.5) give the plain eval's J and dJdu bit for bit; a pulse alone and as pulse 3 of 5 gives the same
    bits; a plain eval before setting and after clearing gives the same bits."""
    from qoc_amd import systems
    prob, _, A0s, As, w, _ = ens_case("cavity")
    u5 = systems.cavity_controls(5, prob.Nt, seed=96)
    e = engine(prob, 5, monkeypatch, W=2, S=16)
    J0, g0, _ = _eval(e, u5, order)
    nom = np.stack([prob.A0, prob.A0]), [np.stack([a, a]) for a in prob.A]
    e.set_generator_ensemble(*nom, (0.5, 0.5))
    Jn, gn, Jm = _eval(e, u5, order)
    assert np.array_equal(Jn, J0) and np.array_equal(gn, g0)
    assert np.array_equal(Jm[:, 0], J0) and np.array_equal(Jm[:, 1], J0)
    e.set_generator_ensemble(A0s, As, w)  # replaces the ensemble
    J5, g5, Jm5 = _eval(e, u5, order)
    e.clear_generator_ensemble()
    assert e.ensemble_size == 0
    J1, g1, _ = _eval(e, u5, order)
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    e.close()
    e1 = engine(prob, 1, monkeypatch, W=2, S=16)
    e1.set_generator_ensemble(A0s, As, w)
    Ja, ga, Jma = _eval(e1, u5[3:4], order)
    e1.close()
    assert np.array_equal(Ja[0], J5[3]) and np.array_equal(ga[0], g5[3]) and np.array_equal(Jma[0], Jm5[3])


def test_more_workgroups_than_compute_units(built_lib, monkeypatch):
    """B = 40, E = 7: 280 workgroups (the shape rule counts B E: more than one per CU) and an odd divisor in v / E;
    parity on pulses 0, 17 and 39, and every pulse's J̄ is the weighted sum of its own member costs."""
    prob, u, *_ = ens_case("many")
    w = weights("many")
    e = engine(prob, u.shape[0], monkeypatch)
    _set(e, "many")
    J, g, Jm = _parity(e, "many", 3, pulses=(0, 17, 39))
    assert np.isfinite(g).all()
    np.testing.assert_allclose(J, Jm @ w, rtol=0, atol=1e-14)
    e.close()


def _raises(code, f, *a, **k):
    from qoc_amd import QOCError
    with pytest.raises(QOCError) as ei:
        f(*a, **k)
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


def test_refusals(built_lib, monkeypatch):
    from qoc_amd import _lib, systems
    lib = built_lib
    prob, u, A0s, As, w, _ = ens_case("cavity")
    B, nu, Nt = u.shape
    # no generators yet (the raw ABI: GrapeEngine sets them in its constructor)
    h = C.c_void_p()
    assert lib.qoc_create(C.byref(h), 0, prob.N, prob.m, nu, Nt, B, _lib.QOC_FP64) == 0
    z = np.zeros(2 * prob.N * prob.N * 2)
    dp = C.POINTER(C.c_double)
    arr = (dp * nu)(*[z.ctypes.data_as(dp)] * nu)
    assert lib.qoc_set_generator_ensemble(h, 2, z.ctypes.data_as(dp), arr, None) == _lib.QOC_ERR_STATE
    assert lib.qoc_ensemble_size(h) == 0 and not lib.qoc_member_costs_dev(h)
    lib.qoc_destroy(h)

    e = engine(prob, B, monkeypatch)
    J0, g0, _ = _eval(e, u)
    bad = A0s.copy()
    bad[1][0, 1] = 1e-3  # rows 0 and 1 are in different blocks (the qubit drive couples i and i + 5)
    bad[1][1, 0] = -1e-3
    _raises(_lib.QOC_ERR_ARG, e.set_generator_ensemble, bad, As, w)
    bad = A0s.copy()
    bad[2][0, 0] += 0.1  # a real diagonal entry: not skew-Hermitian
    _raises(_lib.QOC_ERR_ARG, e.set_generator_ensemble, bad, As, w)
    for ww in ((0.5, -0.1, 0.6), (0.5, np.nan, 0.5), (0.0, 0.0, 0.0), (np.inf, 1.0, 1.0)):
        _raises(_lib.QOC_ERR_ARG, e.set_generator_ensemble, A0s, As, ww)
    assert e.ensemble_size == 0
    J1, g1, _ = _eval(e, u)  # the failed setters changed nothing
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    lam = e.costate(Nt // 2, 1)

    _set(e, "cavity")
    _raises(_lib.QOC_ERR_STATE, e.state, 0)  # states are per member
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
    # an eval the segmented kernel does not take: a co-state source
    e.set_costate_source(np.zeros((B, Nt + 1, prob.N, prob.m), complex))
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    _raises(un, e.eval_spline, c)
    e.set_costate_source(None)
    assert np.isnan(Jd.cpu().numpy()).all() and np.isnan(gd.cpu().numpy()).all()  # the refused calls wrote nothing
    # the co-states of the last plain backward stay readable, before and after an ensemble eval
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    _eval(e, u)
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    _raises(_lib.QOC_ERR_STATE, e.state, 0)
    # set_generators (the same set included) clears the ensemble
    e.set_generators(prob.A0, prob.A)
    assert e.ensemble_size == 0 and e.member_costs_device() == 0
    _raises(_lib.QOC_ERR_STATE, e.member_costs)
    J2, g2, _ = _eval(e, u)
    assert np.array_equal(J2, J0) and np.array_equal(g2, g0)
    e.close()


@pytest.fixture(scope="module")
def zz_callers(built_lib):
    """zz, Nt = 60, ns = 6, B = 4, E = 3 under the trace cost: what the callers of qoc_eval_dev return."""
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
    e.set_spline_basis(Bs)
    Js, dJdc = e.eval_spline(c0)
    best_s = e.allgather_best()
    u0 = np.einsum("tn,bnj->bjt", Bs, c0)
    Ju, gu, _ = _eval(e, u0)
    best_u = e.allgather_best()
    res = minimize_on_device(e, Bs, torch.from_numpy(c0.transpose(0, 2, 1).reshape(B, nu * ns).copy()).cuda(),
                             lower=-0.4, upper=0.4, max_iter=5)
    best_m = e.allgather_best()
    cf = res.c.cpu().numpy().reshape(B, nu, ns).transpose(0, 2, 1)
    J_again = e.eval_spline(cf)[0]
    Jm_again = e.member_costs()
    e.close()
    return dict(Bs=Bs, w=np.asarray(w), Js=Js, dJdc=dJdc, best_s=best_s, Ju=Ju, gu=gu, best_u=best_u,
                f=res.f.cpu().numpy(), best_m=best_m, J_again=J_again, Jm_again=Jm_again)


def test_eval_spline_is_the_spline_map_of_the_ensemble_gradient(zz_callers):
    z = zz_callers
    assert np.abs(z["Js"] - z["Ju"]).max() <= 1e-12 * z["w"].sum()
    for b in range(4):
        ref = z["Bs"].T @ z["gu"][b].T  # ns x nu
        rel = np.linalg.norm(z["dJdc"][b] - ref) / np.linalg.norm(ref)
        print(b, "rel dJdc", rel)
        assert rel <= 1e-10


def test_device_optimiser_minimises_the_ensemble_cost(zz_callers):
    z = zz_callers
    assert np.array_equal(z["f"], z["J_again"])  # f is the ensemble eval at the returned iterates, bit for bit
    assert (z["f"] < z["Js"]).all()              # every seed went down from its start
    np.testing.assert_allclose(z["J_again"], z["Jm_again"] @ z["w"], rtol=0, atol=1e-14)


def test_allgather_best_is_the_argmin_of_the_ensemble_cost(zz_callers):
    z = zz_callers
    for best, J in ((z["best_s"], z["Js"]), (z["best_u"], z["Ju"]), (z["best_m"], z["J_again"])):
        assert best[0] == J.min() and best[1] == int(J.argmin())
