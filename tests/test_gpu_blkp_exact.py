"""The exact (Fréchet) gradient, dUkdp_order = "exact", on the stored / interpolating block propagators of blocks of
5..16 rows with one control (csrc/qoc_blkp.hpp k_blkp_grad_exact): the slice propagators lie on one curve
U(u) = e^{μ(u)} Σ_i T_i(ξ) M_i, and dU/du = e^{μ(u)} Σ_i T_i(ξ) N_i with N_i = μ_1 M_i + xa M'_i is its derivative, so the
exact mode keeps info()["backward"] == "blocks_prop16" in the fused and the split call form, with a state penalty and a
co-state source, for the trace and the z-calibrated cost.  Against oracle/qoc_oracle's block-exponential Fréchet
gradient (grape_eval(..., order="exact")) at the fp64 bar of tests/test_gpu_blk.py: |ΔJ| <= 1e-12,
||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed.  Where the interpolation does not apply (two controls, QOC_BLKP_INTERP=0) and
with QOC_BLKP_EXACT=0 the dense Fréchet kernel runs as before.  B = 3, tgate = 350 Nt / 2000.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from test_gpu_blk import _assert_seed, _block_problem, _eval

pytestmark = pytest.mark.gpu

EX = "exact"
MU = 0.3
B = 3
# the interpolating chains on wave pairs and the upper triangle (default), the full layout, the stored propagators
FORMS = {"triangle": {}, "full": {"QOC_BLKP_ISYM": "0"}, "stored": {"QOC_BLKP_ICHAIN": "0"}}
SWITCHES = ("QOC_BLKP", "QOC_BLKP_PEN", "QOC_BLKP_ICHAIN", "QOC_BLKP_IPAIR", "QOC_BLKP_IPW", "QOC_BLKP_ISYM", "QOC_BLKP_CH",
            "QOC_BLKP_SPLIT", "QOC_BLKP_INTERP", "QOC_BLK_DEAD", "QOC_BLKP_EXACT", "QOC_BLKP_PARTS")


def _rows(labels):
    from qoc_amd import systems
    return [int(r) for r in systems.QuantumBasis([3, 3, 3])(labels)]


def _bus_pen():
    return _rows(["020", "011", "002", "101", "010"]), [0], MU


def _cz_pen():
    return _rows(["200", "020", "002", "110", "011"]), [0, 1, 3], MU


@functools.lru_cache(maxsize=None)
def _case(which, Nt):
    from qoc_amd import systems
    mk = systems.tunable_bus_problem if which == "tunable_bus" else systems.tunable_bus_cz_problem
    prob = mk(Nt=Nt, tgate=350.0 * Nt / 2000)
    u = systems.tunable_bus_controls(B, Nt, seed=100 + Nt)
    u.setflags(write=False)
    return prob, u


@functools.lru_cache(maxsize=None)
def _oracle(which, Nt, pen=None):
    """(J, dJdu, cache) of every seed at order "exact": computed once, shared, never changed."""
    prob, u = _case(which, Nt)
    p = {"bus": _bus_pen(), "cz": _cz_pen(), None: None}[pen]
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=EX, penalty=p) for b in range(B))


def _engine(prob, nseeds, monkeypatch, pen=None, env=None, zcal=False):
    from qoc_amd import GrapeEngine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QOC_BLOCKS", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=nseeds)
    if zcal:
        e.set_cost_zcalibrated(prob.x_target)
    else:
        e.set_cost_trace(prob.x_target, prob.n)
    e.set_chain("taylor")
    if pen is not None:
        e.set_state_penalty(*pen)
    return e


def _assert_batch(J, g, ref, tag):
    for b in range(len(ref)):
        print(tag, b, "dJ", J[b] - ref[b][0], "dg", np.linalg.norm(g[b] - ref[b][1]) / np.linalg.norm(ref[b][1]))
    for b in range(len(ref)):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (tag, b))


def _on_path(e):
    info = e.info()
    assert info["backward"] == "blocks_prop16", info
    return info


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("Nt", [3, 21, 48])
def test_tunable_bus_exact(built_lib, monkeypatch, Nt, form):
    """The tunable bus at m = 1 (one live wave block).  Nt = 3 is shorter than one wave's group of 4 slices, 21 is no
    multiple of it, 48 is.  The fused and the split call form give the same bits (no atomics, one wave per slice)."""
    prob, u = _case("tunable_bus", Nt)
    ref = _oracle("tunable_bus", Nt)
    e = _engine(prob, B, monkeypatch, env=FORMS[form])
    J, g = _eval(e, u, True, order=EX)
    info = _on_path(e)
    assert (info["interp_chain"] > 0) == (form != "stored"), info
    assert (info["interp_chain"] == 2) == (form == "triangle"), info
    _assert_batch(J, g, ref, ("fused", Nt, form))
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, EX)
    info = _on_path(e)
    assert info["split_forward"] == "blocks_prop16", info
    e.close()
    _assert_batch(Js, gs, ref, ("split", Nt, form))
    assert np.array_equal(Js, J) and np.array_equal(gs, g)


@pytest.mark.parametrize("Nt", [21, 48])
def test_cz_exact_trace_cost(built_lib, monkeypatch, Nt):
    """The CZ variant (m = 4, both parity blocks live: two wave blocks, whose coefficients take two launches of the
    gradient kernel when they do not share the LDS), the trace cost, fused and split."""
    prob, u = _case("tunable_bus_cz", Nt)
    ref = _oracle("tunable_bus_cz", Nt)
    e = _engine(prob, B, monkeypatch)
    J, g = _eval(e, u, True, order=EX)
    _on_path(e)
    _assert_batch(J, g, ref, ("cz fused", Nt))
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, EX)
    _on_path(e)
    e.close()
    _assert_batch(Js, gs, ref, ("cz split", Nt))
    assert np.array_equal(Js, J) and np.array_equal(gs, g)


@pytest.mark.parametrize("Nt", [21, 48])
def test_cz_exact_zcalibrated_cost_against_the_dense_path(built_lib, monkeypatch, Nt):
    """The z-calibrated cost on the CZ variant: the exact gradient on the block propagators against the dense Fréchet
    path (QOC_BLKP_EXACT=0) on the same engine settings, J against the oracle's cost of its own x_N."""
    prob, u = _case("tunable_bus_cz", Nt)
    Jz, _ = O.setup_infidelity_zcalibrated(prob.x_target)
    out = {}
    for sw in ("0", None):
        e = _engine(prob, B, monkeypatch, env={"QOC_BLKP_EXACT": sw} if sw else None, zcal=True)
        out[sw] = _eval(e, u, True, order=EX) + (e.info()["backward"],)
        e.close()
    assert out["0"][2] != "blocks_prop16" and out[None][2] == "blocks_prop16", (out["0"][2], out[None][2])
    ref = _oracle("tunable_bus_cz", Nt)
    for b in range(B):
        print("zcal", b, out[None][0][b] - Jz(ref[b][2].x[-1]),
              np.linalg.norm(out[None][1][b] - out["0"][1][b]) / np.linalg.norm(out["0"][1][b]))
    for b in range(B):
        assert abs(out[None][0][b] - Jz(ref[b][2].x[-1])) <= 1e-12
        _assert_seed(out[None][0][b], out[None][1][b], out["0"][0][b], out["0"][1][b], ("zcal", Nt, b))


@pytest.mark.parametrize("NB,nblk,m", [(16, 2, 1), (12, 3, 2), (5, 6, 1)])
def test_random_permuted_blocks_exact(built_lib, monkeypatch, NB, nblk, m):
    """Random skew-Hermitian generators with permuted blocks and one control: non-symmetric generator blocks (the
    full layout), μ_1 != 0, padding rows in the short last block, several live wave blocks."""
    prob, u = _block_problem(NB=NB, nblk=nblk, nu=1, m=m, Nt=40, seed=NB * 7 + nblk + m)
    e = _engine(prob, 2, monkeypatch)
    J, g = _eval(e, u, True, order=EX)
    _on_path(e)
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, EX)
    _on_path(e)
    e.close()
    ref = [O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=EX) for b in range(2)]
    _assert_batch(J, g, ref, (NB, nblk, m))
    assert np.array_equal(Js, J) and np.array_equal(gs, g)


@pytest.mark.parametrize("which", ["tunable_bus", "tunable_bus_cz"])
def test_penalty_exact(built_lib, monkeypatch, which):
    """The state penalty (μ = 0.3, Nt = 21): the penalised forward, the λ chain with its sources, and the exact
    gradient reading λ itself (the LAM instantiation), fused and split."""
    Nt = 21
    prob, u = _case(which, Nt)
    pen = _bus_pen() if which == "tunable_bus" else _cz_pen()
    ref = _oracle(which, Nt, "bus" if which == "tunable_bus" else "cz")
    e = _engine(prob, B, monkeypatch, pen=pen)
    J, g = _eval(e, u, True, order=EX)
    _on_path(e)
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, EX)
    _on_path(e)
    e.close()
    _assert_batch(J, g, ref, ("penalty fused", which))
    _assert_batch(Js, gs, ref, ("penalty split", which))


def test_costate_source_exact(built_lib, monkeypatch):
    """A caller's co-state source dL_dx(x) = 2 W ⊙ x over every row of the m = 1 tunable bus: every block counts as live,
    so the backward forms the propagators -- and the derivative coefficients -- of both parity blocks, a layout the
    propagate did not run on."""
    Nt = 21
    prob, u = _case("tunable_bus", Nt)
    N, m = prob.x0.shape
    W = np.random.default_rng(5).uniform(0.05, 0.4, size=(N, m))
    Jf, dJf = O.setup_infidelity(prob.x_target, prob.n)
    ref = []
    for b in range(B):
        cache = O.setup_grape_cache(prob.A0, prob.x0, u[b].shape)
        x = O.propagate(prob.A0, prob.A, u[b], prob.x0, cache)
        gr = O.grape_sensitivity(prob.A0, prob.A, dJf, cache.u, prob.x0, cache, dUkdp_order=EX, dL_dx=lambda v: 2 * W * v).copy()
        ref.append((Jf(x[-1]), gr, cache))
    src = np.stack([np.stack([2 * W * x for x in ref[b][2].x]) for b in range(B)])
    e = _engine(prob, B, monkeypatch)
    Js = e.propagate(u)
    e.set_costate_source(src)
    gs = e.grape_sensitivity(u, EX)
    _on_path(e)
    _assert_batch(Js, gs, ref, "source split")
    J, g = _eval(e, u, True, order=EX)
    _on_path(e)
    e.close()
    _assert_batch(J, g, ref, "source fused")


def test_control_range_change_on_one_engine(built_lib, monkeypatch):
    """Controls in [0.3, 1.0], then 0.1 + 1.6 (u - 0.3) in [0.1, 1.22], outside the first range and its 5 % margin: the
    derivative coefficients are recomputed with the propagators' (a stale N_i would miss the oracle by orders)."""
    Nt = 21
    prob, u = _case("tunable_bus", Nt)
    u2 = 0.1 + 1.6 * (u - 0.3)
    e = _engine(prob, B, monkeypatch)
    J, g = _eval(e, u, True, order=EX)
    _on_path(e)
    _assert_batch(J, g, _oracle("tunable_bus", Nt), "first range")
    J2, g2 = _eval(e, u2, True, order=EX)
    _on_path(e)
    e.close()
    ref2 = [O.grape_eval(prob.A0, prob.A, u2[b], prob.x0, prob.x_target, prob.n, order=EX) for b in range(B)]
    _assert_batch(J2, g2, ref2, "second range")


@pytest.mark.parametrize("which", ["nu2", "interp0", "exact0"])
def test_fallbacks_keep_the_dense_frechet_path(built_lib, monkeypatch, which):
    """Two controls, QOC_BLKP_INTERP=0 and QOC_BLKP_EXACT=0: the exact mode leaves the block propagators as before and
    still matches the oracle, fused and split; order 3 afterwards is on them again."""
    if which == "nu2":
        prob, u = _block_problem(NB=10, nblk=3, nu=2, m=2)
        env = None
        ref = [O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=EX) for b in range(2)]
    else:
        prob, u = _case("tunable_bus", 21)
        env = {"QOC_BLKP_INTERP": "0"} if which == "interp0" else {"QOC_BLKP_EXACT": "0"}
        ref = _oracle("tunable_bus", 21)
    e = _engine(prob, u.shape[0], monkeypatch, env=env)
    J, g = _eval(e, u, True, order=EX)
    assert e.info()["backward"] != "blocks_prop16", e.info()
    _assert_batch(J, g, ref, ("fused", which))
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, EX)
    assert e.info()["backward"] != "blocks_prop16", e.info()
    _assert_batch(Js, gs, ref, ("split", which))
    _eval(e, u, True, order=3)
    _on_path(e)
    e.close()


def test_unresolved_control_range_takes_the_dense_path(built_lib, monkeypatch):
    """Controls spread over [-1.5, 3.5]: the 40-point series of the propagators' curve does not converge there, so there
    is no curve to differentiate.  The exact eval then is the one of QOC_BLKP_EXACT=0, bit for bit, fused and split
    (decided before anything is launched), and matches the oracle."""
    Nt = 21
    prob, u = _case("tunable_bus", Nt)
    u2 = -1.5 + 5.0 * (u - 0.3) / 0.7
    out = {}
    for sw in ("0", None):
        e = _engine(prob, B, monkeypatch, env={"QOC_BLKP_EXACT": sw} if sw else None)
        J, g = _eval(e, u2, True, order=EX)
        info = e.info()
        assert info["backward"] != "blocks_prop16" and info["interp_degree"] == 0, info
        Js = e.propagate(u2)
        gs = e.grape_sensitivity(u2, EX)
        assert e.info()["backward"] != "blocks_prop16", e.info()
        e.close()
        out[sw] = (J, g, Js, gs)
    for a, r in zip(out[None], out["0"]):
        assert np.array_equal(a, r)
    ref = [O.grape_eval(prob.A0, prob.A, u2[b], prob.x0, prob.x_target, prob.n, order=EX) for b in range(B)]
    _assert_batch(out[None][0], out[None][1], ref, "wide range")


@pytest.mark.parametrize("form", ["triangle", "stored"])
def test_stale_u_exact(built_lib, monkeypatch, form):
    """grape_sensitivity(u2, "exact") after propagate(u): "Cache data from other control signal u"; on the device entry
    point the exact gradient kernel reads the queued flag itself and leaves the caller's buffer as it was."""
    import torch
    from qoc_amd import StaleCacheError
    Nt = 21
    prob, u = _case("tunable_bus", Nt)
    e = _engine(prob, B, monkeypatch, env=FORMS[form])
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    u2 = ud.clone()
    u2[1, 5, 0] += 1e-9
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.full((B, Nt, 1), 7.0, dtype=torch.float64, device="cuda")
    e.propagate_device(ud.data_ptr(), Jd.data_ptr())
    with pytest.raises(StaleCacheError):
        e.grape_sensitivity_device(u2.data_ptr(), EX, gd.data_ptr())
    e.synchronize()
    assert bool((gd == 7.0).all())
    e.grape_sensitivity_device(ud.data_ptr(), EX, gd.data_ptr())
    e.synchronize()
    _on_path(e)
    _assert_batch(Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), _oracle("tunable_bus", Nt), ("after stale", form))
    # the host entry points
    e.propagate(u)
    uh = np.array(u)
    uh[1, 0, 5] += 1e-9
    with pytest.raises(StaleCacheError):
        e.grape_sensitivity(uh, EX)
    e.close()


def test_exact_is_the_derivative_of_the_computed_cost(built_lib, monkeypatch):
    """Nt = 48, the first seed of tunable_bus_controls(., 48, seed=81): central differences of the device's own J along a
    unit direction from default_rng(5) (h = 1e-6; u, u + h d, u - h d in one batch) against g·d.  The exact gradient
    meets them to 1e-6 relative (the CPU oracle: fd -0.0222872356, g_exact·d -0.0222872357); order 3 from the same
    engine gives +2.76 (||A_k||_1 ~ 30: the truncated series of expm_jacobian! is not small), which is why the mode
    exists."""
    from qoc_amd import systems
    Nt = 48
    prob = systems.tunable_bus_problem(Nt=Nt, tgate=350.0 * Nt / 2000)
    u = systems.tunable_bus_controls(B, Nt, seed=81)[:1]
    d = np.random.default_rng(5).standard_normal(u.shape)
    d /= np.linalg.norm(d)
    h = 1e-6
    e = _engine(prob, 3, monkeypatch)
    J, g = _eval(e, np.concatenate([u, u + h * d, u - h * d]), True, order=EX)
    _on_path(e)
    _, g3 = _eval(e, np.concatenate([u, u, u]), True, order=3)
    e.close()
    fd = (J[1] - J[2]) / (2 * h)
    dex, d3 = float(np.sum(g[0] * d[0])), float(np.sum(g3[0] * d[0]))
    print(f"fd {fd:.10e} exact {dex:.10e} order 3 {d3:.10e}")
    assert abs(dex - fd) <= 1e-6 * abs(fd), (dex, fd)
    assert abs(d3 - fd) > 1e-6 * abs(fd), (d3, fd)


def test_exact_device_optimiser_on_the_block_propagators(built_lib, monkeypatch):
    """The device-resident optimiser at order "exact" on the small bus (Nt = 48, 8 splines, B = 3, bounds [0.3, 1.0])
    against the host state machine driven by SplineGrape(order="exact"), with the checks of
    tests/test_gpu_blkseg_exact.py's zz run; the evals behind both stay on the block propagators."""
    import torch
    from qoc_amd import GrapeEngine, systems
    from qoc_amd.optimize import SplineGrape, minimize_on_device, minimize_ticks
    for k in SWITCHES + ("QOC_BLOCKS",):
        monkeypatch.delenv(k, raising=False)
    Nt = 48
    tgate = 350.0 * Nt / 2000
    prob = systems.tunable_bus_problem(Nt=Nt, tgate=tgate)
    Bs = systems.spline_matrix(tgate, Nt, 8)
    ns = Bs.shape[1]
    c0 = np.random.default_rng(1).uniform(0.4, 0.9, size=(B, ns))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    kw = dict(lower=0.3, upper=1.0, max_iter=8, outer_iters=1)
    sg = SplineGrape(e, Bs, order=EX)
    c0d = torch.from_numpy(c0).to("cuda:0")
    ref = minimize_ticks(sg.fg, c0d, **kw)
    _on_path(e)
    dev = minimize_on_device(e, Bs, c0d, order=EX, **kw)
    _on_path(e)
    e.close()
    assert dev.evals.tolist() == ref.evals.tolist()
    assert dev.ticks == int(ref.evals.max()) == ref.ticks == dev.n_evals
    assert dev.not_done == 0 and bool(dev.done.all()) and dev.history == []
    d = {k: float((getattr(dev, k) - getattr(ref, k)).abs().max()) for k in ("c", "f")}
    print(f"max |dc| = {d['c']:.3e}, |df| = {d['f']:.3e}, evals {dev.evals.tolist()}")
    assert d["c"] <= 1e-8 and d["f"] <= 1e-10  # (no constraints here: no multipliers to compare)
    assert dev.iters.tolist() == ref.iters.tolist() and dev.rounds.tolist() == ref.rounds.tolist()
