"""GPU: the gate duration as a per-seed variable (include/qoc.h qoc_set_time_scale; the TS instantiations of
k_blkseg_eval, csrc/qoc_blkseg.hpp).

With a time scale set, seed b evolves under τ_b (A0 + Σ_j u_jk A_j); eval_device returns J_b and dJ_b/du_b at fixed
τ_b and leaves dJ_b/dτ_b at fixed u_b in the engine's buffer.  The reference is tests/duration_util.py: the oracle on
the scaled generators and dJ/dτ = Σ_k Re<λ_{k+1}, A_k x_{k+1}>; the bars are |ΔJ| <= 1e-12 max(1, |J|),
||ΔdJdu|| / ||dJdu|| <= 1e-10 and |ΔdJ/dτ| <= 1e-10 S with S = Σ_k |term|, all scales from the reference.  Every test
here needs the new entry points, so none passes without them.

The τ values come from ρ_max = rad_0 + Σ|u| rad_j on the CPU (≈ 0.12 for cavity20, ≈ 0.19-0.24 for zz at τ = 1): they
are meant to land a seed in each of blkseg_series_k's classes (ρ <= 0.24, <= 0.66, <= θ_cap ≈ 0.98) and past θ_cap, so
that one launch mixes the fast loops at K = 5, 7, 9 with the generic loop with halvings.  The classes are intent,
not asserted.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import block_problem, bufs, case, dev, engine, pen
from duration_util import EX, assert_seed, reference
from ensemble_util import ens_case

pytestmark = pytest.mark.gpu


def _eval(e, u, order=3):
    """eval_device on fresh NaN-filled buffers -> J (B,), dJdu (B, nu, Nt), dJ/dτ (B,)."""
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), e.time_scale_grad()


def _plain(e, u, order=3):
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1))


def _parity(e, key, prob, u, tau, order, zcal=False, penalty=None, seeds=None):
    e.set_time_scale(tau)
    J, g, d = _eval(e, u, order)
    assert np.isfinite(d).all()
    for b in (range(u.shape[0]) if seeds is None else seeds):
        ref = reference((key, b), prob, u[b], tau[b], order, zcal, penalty)
        assert_seed(J[b], g[b], d[b], ref, (key, order, b, tau[b]), (prob, u[b], tau[b], order) if zcal else None)
    return J, g, d


@pytest.mark.parametrize("order", [1, 2, 3, 4, EX])
def test_blocks_of_2_zero_diagonal(built_lib, monkeypatch, order):
    """cavity20 (N = 20, 10 blocks of 2, Nt = 50), four seeds: pulses 0, 1, 2, 0 at τ = (1, 3.5, 7, 14): the phase-free
    SU(2) loops at three series degrees and the generic loop with halvings in one launch."""
    prob, u3, _ = case("cavity20")
    u = u3[[0, 1, 2, 0]]
    e = engine(prob, 4, monkeypatch)
    _parity(e, "cavity20", prob, u, np.array([1.0, 3.5, 7.0, 14.0]), order)
    e.close()


@pytest.mark.parametrize("order", [3, EX])
@pytest.mark.parametrize("name", ["sigma_z", "nominal"])
def test_blocks_of_2_general_form_and_tails(built_lib, monkeypatch, name, order):
    """N_cavity = 5, Nt = 37 (segment tails): the generator set of ens_case("mixed") member 1, whose first control has a
    σ_z part (the general 2-row form), and ens_case("cavity")'s nominal problem (zero-diagonal class), each with its
    own pulses."""
    if name == "sigma_z":
        p, u, A0s, As, _, _ = ens_case("mixed")
        prob = dataclasses.replace(p, A0=A0s[1], A=[a[1] for a in As])
    else:
        prob, u, *_ = ens_case("cavity")
    e = engine(prob, u.shape[0], monkeypatch)
    _parity(e, "cavity5_" + name, prob, u, np.array([0.6, 1.0, 1.7]), order)
    e.close()


@pytest.mark.parametrize("order,zcal", [(1, False), (2, False), (3, False), (4, False), (EX, False), (3, True), (EX, True)])
def test_blocks_of_3(built_lib, monkeypatch, order, zcal):
    """zz (N = 9, 3 blocks of 3, Nt = 60, m = 4) at τ = (0.7, 2, 8): the generic loop without and with halvings, the
    trace cost at every order and the z-calibrated cost."""
    prob, u, _ = case("zz")
    e = engine(prob, u.shape[0], monkeypatch)
    if zcal:
        e.set_cost_zcalibrated(prob.x_target)
    _parity(e, "zz", prob, u, np.array([0.7, 2.0, 8.0]), order, zcal)
    e.close()


@pytest.mark.parametrize("order", [3, EX])
@pytest.mark.parametrize("shape,seed", [((3, 3, 2, 2), 11), ((2, 4, 1, 2), 12)])
def test_permuted_blocks_with_a_padding_row(built_lib, monkeypatch, shape, seed, order):
    NB, nblk, nu, m = shape
    prob, u, _ = block_problem(NB, nblk, nu, m, 23, seed)
    e = engine(prob, 2, monkeypatch)
    _parity(e, ("blocks", shape, seed), prob, u, np.array([0.8, 1.9]), order)
    e.close()


@pytest.mark.parametrize("order", [3, EX])
def test_penalty_on_blocks_of_2(built_lib, monkeypatch, order):
    """cavity20 with its penalty: the one-launch penalised kernel; J includes Σ_k L(x_k), dJ/dτ the sources of λ."""
    prob, u3, pn = case("cavity20")
    u = u3[[0, 1, 2, 0]]
    e = engine(prob, 4, monkeypatch, pen=pen(pn))
    _parity(e, "cavity20", prob, u, np.array([1.0, 3.5, 7.0, 14.0]), order, penalty=pn)
    e.close()


@pytest.mark.parametrize("order", [1, 3, EX])
def test_penalty_on_blocks_of_3(built_lib, monkeypatch, order):
    """zz with its guard-state penalty: the forward and the backward half as two launches (what a sweep exists for:
    shorter gates drive harder and leak more into |20>, |21>, |22>)."""
    prob, u, pn = case("zz")
    e = engine(prob, u.shape[0], monkeypatch, pen=pen(pn))
    _parity(e, "zz", prob, u, np.array([0.7, 2.0, 8.0]), order, penalty=pn)
    e.close()


def test_indexing_with_more_workgroups_than_a_wave(built_lib, monkeypatch):
    """N_cavity = 3, Nt = 16, B = 40, τ_b = 0.5 + 0.05 b: parity on seeds 0, 17, 39 and every dJ/dτ finite."""
    from qoc_amd import systems
    prob = systems.cavity_problem(N_cavity=3, Nt=16)
    u = systems.cavity_controls(40, 16, seed=94)
    e = engine(prob, 40, monkeypatch)
    _parity(e, "cavity3", prob, u, 0.5 + 0.05 * np.arange(40), 3, seeds=(0, 17, 39))
    e.close()


@pytest.mark.parametrize("order", [3, EX])
@pytest.mark.parametrize("name", ["cavity", "zz"])
def test_bitwise(built_lib, monkeypatch, name, order):
    """With the launch shape pinned (QOC_BLKSEG_W = 2, QOC_BLKSEG_S = 16): τ ≡ 1 gives the plain eval's J and dJdu bit
    for bit; a seed alone and as seed 3 of 5 (the others at other τ) gives the same J, dJdu and dJ/dτ bits; τ written
    through time_scale_device() gives the bits of the host setter; after clearing, the plain eval is the one before."""
    import torch
    from qoc_amd import systems
    from qoc_amd.optimize import _DevView
    if name == "cavity":
        prob = ens_case("cavity")[0]
        u5 = systems.cavity_controls(5, prob.Nt, seed=96)
    else:
        prob = case("zz")[0]
        u5 = systems.zz_controls(5, prob.Nt, 6.0, seed=98)
    tau5 = np.array([0.7, 1.3, 0.9, 1.6, 1.1])
    e = engine(prob, 5, monkeypatch, W=2, S=16)
    J0, g0 = _plain(e, u5, order)
    e.set_time_scale(np.ones(5))
    J1, g1, _ = _eval(e, u5, order)
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    e.set_time_scale(tau5)
    J5, g5, d5 = _eval(e, u5, order)
    assert not np.array_equal(J5, J0)
    # the device pointer: back to ones through the setter, then τ written into the engine's buffer
    e.set_time_scale(np.ones(5))
    view = torch.as_tensor(_DevView(e.time_scale_device(), (5,), "<f8"), device="cuda")
    view.copy_(torch.from_numpy(tau5))
    torch.cuda.synchronize()
    Jp, gp, dp = _eval(e, u5, order)
    assert np.array_equal(Jp, J5) and np.array_equal(gp, g5) and np.array_equal(dp, d5)
    e.set_time_scale(None)
    assert e.time_scale_device() == 0 and e.time_scale_grad_device() == 0
    J2, g2 = _plain(e, u5, order)
    assert np.array_equal(J2, J0) and np.array_equal(g2, g0)
    assert e.info()["backward"] == "segmented"
    e.close()
    e1 = engine(prob, 1, monkeypatch, W=2, S=16)
    e1.set_time_scale(tau5[3:4])
    Ja, ga, da = _eval(e1, u5[3:4], order)
    e1.close()
    assert np.array_equal(Ja[0], J5[3]) and np.array_equal(ga[0], g5[3]) and np.array_equal(da[0], d5[3])


@pytest.fixture(scope="module")
def zz_callers(built_lib):
    """zz, Nt = 60, ns = 6, B = 4, τ = (0.8, 1, 1.25, 1.6) under the trace cost: what the callers of qoc_eval_dev return."""
    import torch
    from qoc_amd import GrapeEngine, systems
    from qoc_amd.optimize import SplineGrapeDuration, minimize_on_device, minimize_ticks
    prob = case("zz")[0]
    B, ns, nu = 4, 6, 2
    tau = np.array([0.8, 1.0, 1.25, 1.6])
    Bs = systems.spline_matrix(6.0, prob.Nt, ns)
    c0 = np.random.default_rng(97).uniform(-0.3, 0.3, size=(B, ns, nu))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    e.set_chain("taylor")
    e.set_time_scale(tau)
    e.set_spline_basis(Bs)
    Js, dJdc = e.eval_spline(c0)
    best_s = e.allgather_best()
    u0 = np.einsum("tn,bnj->bjt", Bs, c0)
    Ju, gu, du = _eval(e, u0)
    flat0 = c0.transpose(0, 2, 1).reshape(B, nu * ns).copy()
    res = minimize_on_device(e, Bs, torch.from_numpy(flat0).cuda(), lower=-0.4, upper=0.4, max_iter=5)
    best_m = e.allgather_best()
    cf = res.c.cpu().numpy().reshape(B, nu, ns).transpose(0, 2, 1)
    J_again = e.eval_spline(cf)[0]
    # the duration as a variable of the host-driven optimiser
    kappa = 0.05
    obj = SplineGrapeDuration(e, Bs, order=3, time_weight=kappa)
    z0 = torch.from_numpy(np.concatenate([flat0, tau[:, None]], 1)).cuda()
    f0, g0 = (a.cpu().numpy() for a in obj.fg(z0))
    lo = np.concatenate([np.full(nu * ns, -0.4), [0.5]])
    hi = np.concatenate([np.full(nu * ns, 0.4), [2.0]])
    rt = minimize_ticks(obj.fg, z0, lower=lo, upper=hi, max_iter=5)
    e.close()
    return dict(prob=prob, Bs=Bs, tau=tau, c0=c0, u0=u0, Js=Js, dJdc=dJdc, best_s=best_s, Ju=Ju, gu=gu, du=du,
                f=res.f.cpu().numpy(), cf=cf, best_m=best_m, J_again=J_again, kappa=kappa, f0=f0, g0=g0,
                ft=rt.f.cpu().numpy(), zt=rt.c.cpu().numpy())


def test_eval_spline_is_the_spline_map_of_the_scaled_gradient(zz_callers):
    z = zz_callers
    assert np.abs(z["Js"] - z["Ju"]).max() <= 1e-12  # (u from the device's spline map against numpy's: J of order 1)
    for b in range(4):
        ref = z["Bs"].T @ z["gu"][b].T  # ns x nu
        rel = np.linalg.norm(z["dJdc"][b] - ref) / np.linalg.norm(ref)
        print(b, "rel dJdc", rel)
        assert rel <= 1e-10
    assert z["best_s"][0] == z["Js"].min() and z["best_s"][1] == int(z["Js"].argmin())


def test_device_optimiser_runs_a_sweep_as_one_batch(zz_callers):
    z = zz_callers
    assert np.array_equal(z["f"], z["J_again"])  # f is the eval at the returned iterates, bit for bit
    assert (z["f"] < z["Js"]).all()              # every seed went down from its start
    assert z["best_m"][0] == z["f"].min() and z["best_m"][1] == int(z["f"].argmin())
    prob = z["prob"]
    uf = np.einsum("tn,bnj->bjt", z["Bs"], z["cf"])
    for b in range(4):  # the returned f is the cost on that seed's τ-scaled generators
        t = z["tau"][b]
        Jr = O.grape_eval(t * prob.A0, [t * a for a in prob.A], uf[b], prob.x0, prob.x_target, prob.n)[0]
        print(b, "dJ", z["f"][b] - Jr)
        assert abs(z["f"][b] - Jr) <= 1e-12 * max(1.0, abs(Jr))


def test_spline_grape_duration_gradient(zz_callers):
    z = zz_callers
    prob, ns, nu = z["prob"], 6, 2
    for b in range(4):
        Jr, gr, dr, S = reference(("zz_spline", b), prob, z["u0"][b], z["tau"][b], 3)
        assert abs(z["f0"][b] - z["kappa"] * z["tau"][b] - Jr) <= 1e-12 * max(1.0, abs(Jr))
        ref = (z["Bs"].T @ gr.T).T.reshape(nu * ns)  # index s + ns j
        rel = np.linalg.norm(z["g0"][b, :-1] - ref) / np.linalg.norm(ref)
        print(b, "rel dJdc", rel, "ddJdtau / S", (z["g0"][b, -1] - z["kappa"] - dr) / S)
        assert rel <= 1e-10
        assert abs(z["g0"][b, -1] - z["kappa"] - dr) <= 1e-10 * S
        assert abs(z["du"][b] - dr) <= 1e-10 * S


def test_minimize_ticks_with_the_duration_as_a_variable(zz_callers):
    z = zz_callers
    assert (z["ft"] < z["f0"]).all()
    assert (z["zt"][:, -1] >= 0.5).all() and (z["zt"][:, -1] <= 2.0).all()
    assert (np.abs(z["zt"][:, :-1]) <= 0.4).all()


def _raises(code, f, *a, **k):
    from qoc_amd import QOCError
    with pytest.raises(QOCError) as ei:
        f(*a, **k)
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))
    return str(ei.value)


def test_refusals(built_lib, monkeypatch):
    from qoc_amd import GrapeEngine, _lib, systems
    from test_gpu_compress import _block_problem
    prob, u, A0s, As, w, _ = ens_case("cavity")
    B, nu, Nt = u.shape
    un, st, ar = _lib.QOC_ERR_UNSUPPORTED, _lib.QOC_ERR_STATE, _lib.QOC_ERR_ARG
    tau = np.array([0.8, 1.0, 1.3])

    e = engine(prob, B, monkeypatch)
    J0, g0 = _plain(e, u)
    lam = e.costate(Nt // 2, 1)
    info0 = e.info()["device_bytes"]
    for bad in (0.0, -1.0, np.nan, np.inf):
        _raises(ar, e.set_time_scale, np.array([1.0, bad, 1.0]))
    assert e.time_scale_device() == 0 and e.info()["device_bytes"] == info0
    J1, g1 = _plain(e, u)  # the failed setters changed nothing
    assert np.array_equal(J1, J0) and np.array_equal(g1, g0)
    # the two setter orders with an ensemble: the earlier setting stays
    e.set_generator_ensemble(A0s, As, w)
    assert "ensemble" in _raises(un, e.set_time_scale, tau)
    assert e.ensemble_size == 3 and e.time_scale_device() == 0
    e.clear_generator_ensemble()
    _plain(e, u)
    lam = e.costate(Nt // 2, 1)
    e.set_time_scale(tau)
    assert e.info()["device_bytes"] >= info0 + 2 * B * 8
    assert "time scale" in _raises(un, e.set_generator_ensemble, A0s, As, w)
    assert e.ensemble_size == 0 and e.time_scale_device() != 0
    _raises(st, e.time_scale_grad)  # no eval under the scale yet
    _raises(st, e.state, 0)         # the setter invalidated the last forward

    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    Bs = systems.spline_matrix(float(Nt), Nt, 4)
    e.set_spline_basis(Bs)
    c = np.zeros((B, 4, nu))
    par = np.tile([float(Nt), 5.0, 0.01, 0.1], (B, 1))
    for f, a in ((e.propagate, (u,)), (e.grape_sensitivity, (u,)), (e.propagate_device, (ud.data_ptr(), Jd.data_ptr())),
                 (e.grape_sensitivity_device, (ud.data_ptr(), 3, gd.data_ptr())), (e.propagate_spline, (c,)),
                 (e.sensitivity_spline, (c,)), (e.propagate_envelope, ("drag", par, float(Nt), 0.5)),
                 (e.eval_envelope, ("drag", par, float(Nt), 0.5)),
                 (e.eval_envelope_device, ("drag", ud.data_ptr(), 4, float(Nt), 0.5, Jd.data_ptr(), gd.data_ptr()))):
        assert "time scale" in _raises(un, f, *a)
    # evals the segmented kernel does not take: a co-state source, QOC_BLKSEG=0, Tsit5; the external cost
    e.set_costate_source(np.zeros((B, Nt + 1, prob.N, prob.m), complex))
    assert "time scale" in _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    _raises(un, e.eval_spline, c)
    e.set_costate_source(None)
    monkeypatch.setenv("QOC_BLKSEG", "0")
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    monkeypatch.setenv("QOC_BLKSEG", "1")
    e.set_propagation("tsit5", 4)
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.set_propagation("expm")
    e.set_cost_external()
    _raises(st, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.set_cost_trace(prob.x_target, prob.n)
    _raises(ar, e.eval_device, ud.data_ptr(), 7, Jd.data_ptr(), gd.data_ptr())
    assert np.isnan(Jd.cpu().numpy()).all() and np.isnan(gd.cpu().numpy()).all()  # the refused calls wrote nothing
    _raises(st, e.time_scale_grad)
    # the co-states of the last plain backward stay readable, before and after an eval under the scale
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    J, g, d = _eval(e, u)
    assert np.isfinite(d).all() and e.info()["backward"] == "segmented"
    assert np.array_equal(e.costate(Nt // 2, 1), lam)
    _raises(st, e.state, 0)
    # the setting survives set_generators, set_x0 and set_cost
    e._gen_key = None  # so that the same set reaches the library
    e.set_generators(prob.A0, prob.A)
    e.set_x0(prob.x0)
    e.set_cost_trace(prob.x_target, prob.n)
    assert e.time_scale_device() != 0
    Jb, gb, db = _eval(e, u)
    assert np.array_equal(Jb, J) and np.array_equal(gb, g) and np.array_equal(db, d)
    bytes_set = e.info()["device_bytes"]
    e.set_time_scale(None)
    assert e.info()["device_bytes"] == bytes_set - 2 * B * 8  # the 2 B doubles are freed on clear
    J2, g2 = _plain(e, u)
    assert np.array_equal(J2, J0) and np.array_equal(g2, g0)
    e.close()

    # QOC_CONCURRENT=0 is read when the context is made
    monkeypatch.setenv("QOC_CONCURRENT", "0")
    e = engine(prob, B, monkeypatch)
    e.set_time_scale(tau)
    _raises(un, e.eval_device, ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.close()
    monkeypatch.delenv("QOC_CONCURRENT")
    # an fp32 context refuses the setter
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B, precision="fp32")
    _raises(un, e.set_time_scale, tau)
    e.close()
    # generators without blocks of 2-3 rows, and compress_states packing
    bp, v, ub = _block_problem(seed=13)
    for packing in (None, v):
        e = GrapeEngine(bp.A0, bp.A, bp.x0, bp.Nt, B=ub.shape[0])
        e.set_cost_trace(bp.x_target, bp.n)
        if packing is not None:
            e.set_compression(packing)
        e.set_time_scale(np.full(ub.shape[0], 1.2))
        udb = dev(ub)
        Jb_, gb_ = bufs(*[ub.shape[i] for i in (0, 2, 1)])
        _raises(un, e.eval_device, udb.data_ptr(), 3, Jb_.data_ptr(), gb_.data_ptr())
        assert np.isnan(Jb_.cpu().numpy()).all() and np.isnan(gb_.cpu().numpy()).all()
        e.close()
    assert np.isnan(Jd.cpu().numpy()).all() and np.isnan(gd.cpu().numpy()).all()
