"""The state penalty (setup_state_penalty, src/penalty_fcns.jl:1-11) and a caller's co-state source (the dL_dx closure of
grape_sensitivity, src/gradient_computations.jl:47-49, 55-57) on the stored and the interpolating block propagators of
blocks of 5..16 rows (csrc/qoc_blkp.hpp, the PEN instantiations of k_blkp_chain / k_blkp_ichain / k_blkp_ichain2 and
k_blkp_grad's λ mode):
  J = Jfinal(x_N) + Σ_{k=0..Nt} μ Σ_{r in P, c in C} |x_k[r, c]|²,  λ_N = dJfinal/dx(x_N) + s_N,  λ_k = U_k^H λ_{k+1} + s_k,
  s_k = 2μ x_k[P, C] + the caller's source of slice k.
Against oracle/qoc_oracle (grape_eval(..., penalty=...), grape_sensitivity(..., dL_dx=...)) and the Chebyshev block
chains (QOC_BLKP_PEN=0) at the fp64 bar of tests/test_gpu_blkp.py: |ΔJ| <= 1e-12, ||ΔdJdu|| / ||dJdu|| <= 1e-10 per
seed, co-states within 1e-12 of the oracle's largest entry.  B = 3, tgate = 350 Nt / 2000, μ = 0.3: the penalty is
0.15..3.8 of J there and multiplies the gradient's norm 30..200 times, so a wrong or missing term cannot pass.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from test_gpu_blk import _assert_seed, _block_problem, _eval

pytestmark = pytest.mark.gpu

MU = 0.3
B = 3
# interpolating chains: two waves per chain (default), one wave; the stored propagators
FORMS = {"pair": {}, "single": {"QOC_BLKP_IPAIR": "0"}, "stored": {"QOC_BLKP_ICHAIN": "0"}}
SWITCHES = ("QOC_BLKP", "QOC_BLKP_PEN", "QOC_BLKP_ICHAIN", "QOC_BLKP_IPAIR", "QOC_BLKP_IPW", "QOC_BLKP_ISYM", "QOC_BLKP_CH",
            "QOC_BLKP_SPLIT", "QOC_BLKP_INTERP", "QOC_BLK_DEAD")


def _rows(labels):
    from qoc_amd import systems
    return [int(r) for r in systems.QuantumBasis([3, 3, 3])(labels)]


def _bus_pen():
    """|010> lies in the odd block, which carries no state of |110> -> |200> (a dead block)."""
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
    return prob, u, (_bus_pen() if which == "tunable_bus" else _cz_pen())


@functools.lru_cache(maxsize=None)
def _oracle(which, Nt, penalised=True):
    """(J, dJdu, cache) of every seed: computed once, shared, never changed."""
    prob, u, pen = _case(which, Nt)
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3,
                              penalty=pen if penalised else None) for b in range(B))


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


def _assert_costates(e, cache, b, ks, tag):
    lsc = max(np.abs(lam).max() for lam in cache.lam)
    for k in ks:
        d = np.abs(e.costate(k, seed=b) - cache.lam[k]).max()
        print(tag, "costate", k, d / lsc)
        assert d <= 1e-12 * lsc, (tag, "lambda", b, k, d / lsc)


def _assert_batch(J, g, ref, tag):
    for b in range(len(ref)):
        print(tag, b, "dJ", J[b] - ref[b][0], "dg", np.linalg.norm(g[b] - ref[b][1]) / np.linalg.norm(ref[b][1]))
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (tag, b))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("Nt", [3, 21, 48])
def test_tunable_bus_penalty(built_lib, monkeypatch, Nt, form):
    """The tunable bus at m = 1 (one live wave block: the interpolating chains, two waves or one per chain, and the
    stored form).  Nt = 3 is shorter than a chunk of 8 slices; Nt = 21 is no multiple of any chunk size and gives the
    wave pairs an odd chunk count.  The fused and the split call form, co-states at both ends and in the middle."""
    prob, u, pen = _case("tunable_bus", Nt)
    ref = _oracle("tunable_bus", Nt)
    if Nt >= 21:  # the penalty's share of J, from the oracle's own states
        L, _ = O.setup_state_penalty(*pen)
        assert min(sum(L(x) for x in ref[b][2].x) for b in range(B)) > 0.1
    e = _engine(prob, B, monkeypatch, pen=pen, env=FORMS[form])
    J, g = _eval(e, u, True)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    assert (info["interp_chain"] > 0) == (form != "stored"), info
    _assert_batch(J, g, ref, ("fused", Nt, form))
    _assert_costates(e, ref[1][2], 1, (0, Nt // 2, Nt), ("fused", Nt, form))
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, 3)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    assert (info["interp_chain"] > 0) == (form != "stored"), info
    _assert_batch(Js, gs, ref, ("split", Nt, form))
    _assert_costates(e, ref[2][2], 2, (0, Nt // 2, Nt), ("split", Nt, form))
    e.close()


@pytest.mark.parametrize("Nt", [21, 48])
def test_cz_penalty_stored_propagators(built_lib, monkeypatch, Nt):
    """The CZ variant (m = 4, x0 columns in both parity blocks: two live wave blocks, 8 chain waves per seed) on the
    stored propagators: the penalty sum over the waves of a workgroup, three of the four columns penalised."""
    prob, u, pen = _case("tunable_bus_cz", Nt)
    ref = _oracle("tunable_bus_cz", Nt)
    L, _ = O.setup_state_penalty(*pen)
    assert min(sum(L(x) for x in ref[b][2].x) for b in range(B)) > 0.1
    e = _engine(prob, B, monkeypatch, pen=pen)
    J, g = _eval(e, u, True)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    _assert_batch(J, g, ref, ("cz fused", Nt))
    _assert_costates(e, ref[0][2], 0, (0, Nt // 2, Nt), ("cz fused", Nt))
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, 3)
    assert e.info()["backward"] == "blocks_prop16", e.info()
    _assert_batch(Js, gs, ref, ("cz split", Nt))
    e.close()


def test_cz_penalty_zcalibrated_cost(built_lib, monkeypatch):
    """The z-calibrated cost with the penalty on the CZ variant: J against the oracle's cost of its own x_N plus the
    penalty's sum; the gradient less the penalty's own part (linear in the source; the oracle's, with a zero final
    cost) against the oracle's family g(Δθ) within the calibration phase's bound, as tests/test_gpu_blkseg.py holds it."""
    Nt = 21
    prob, u, pen = _case("tunable_bus_cz", Nt)
    Jz, _ = O.setup_infidelity_zcalibrated(prob.x_target)
    Lf, _ = O.setup_state_penalty(*pen)
    e = _engine(prob, B, monkeypatch, pen=pen, zcal=True)
    J, g = _eval(e, u, True)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    e.close()
    zero = (lambda x: 0.0, lambda x: np.zeros_like(np.asarray(x, dtype=complex)))
    for b in range(B):
        xs = _oracle("tunable_bus_cz", Nt)[b][2].x
        print("zcal", b, J[b] - (Jz(xs[-1]) + sum(Lf(x) for x in xs)))
        assert abs(J[b] - (Jz(xs[-1]) + sum(Lf(x) for x in xs))) <= 1e-12
        gpen = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=3, penalty=pen, cost=zero)[1]
        res, dth = O.zcal_gradient_match(g[b] - gpen, prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=3)
        print("zcal", b, res, dth)
        assert res <= 1e-10 and abs(dth) <= O.zcal_dtheta_bound(prob.x_target, xs[-1]), (b, res, dth)


@pytest.mark.parametrize("NB,nblk,nu,m", [(10, 3, 2, 2), (16, 2, 1, 1), (7, 4, 2, 2)])
def test_random_permuted_blocks_penalty(built_lib, monkeypatch, NB, nblk, nu, m):
    """Random skew-Hermitian generators with permuted blocks (a short last block: padding rows), nu = 2 (k_blkp_exp)
    and nu = 1 with two live blocks (k_blkp_int + the stored chains)."""
    prob, u = _block_problem(NB=NB, nblk=nblk, nu=nu, m=m, Nt=40, seed=NB * 7 + nblk + nu + m)
    pen = ([0, 3, 5], [0], MU)
    e = _engine(prob, 2, monkeypatch, pen=pen)
    J, g = _eval(e, u, True)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    ref = [O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3, penalty=pen) for b in range(2)]
    _assert_batch(J, g, ref, (NB, nblk, nu, m))
    _assert_costates(e, ref[1][2], 1, (0, 20, 40), (NB, nblk, nu, m))
    e.close()


def _source_reference(prob, u_b, W, pen):
    """The oracle's propagate + grape_sensitivity with dL_dx(x) = 2 W ⊙ x (+ the state penalty's): the states the
    source is built from, J, dJdu and the cache with λ_k."""
    Jf, dJf = O.setup_infidelity(prob.x_target, prob.n)
    L = dLp = None
    if pen is not None:
        L, dLp = O.setup_state_penalty(*pen)
    cache = O.setup_grape_cache(prob.A0, prob.x0, u_b.shape)
    x = O.propagate(prob.A0, prob.A, u_b, prob.x0, cache)
    dL = (lambda v: 2 * W * v) if dLp is None else (lambda v: 2 * W * v + dLp(v))
    g = O.grape_sensitivity(prob.A0, prob.A, dJf, cache.u, prob.x0, cache, dUkdp_order=3, dL_dx=dL).copy()
    J = Jf(x[-1]) + (sum(L(xk) for xk in x) if L is not None else 0.0)
    return J, g, cache


@pytest.mark.parametrize("which", ["tunable_bus", "blocks"])
@pytest.mark.parametrize("with_pen", [False, True])
def test_costate_source(built_lib, monkeypatch, which, with_pen):
    """A weighted field over every row and column, dL_dx(x) = 2 W ⊙ x with W random positive, built from the oracle's
    states, alone and with the state penalty: every block counts as live (the m = 1 tunable bus then runs the stored
    chains on both parity blocks), dJdu and λ_k on all rows (the odd block's included) in the split form (the source
    set between propagate and grape_sensitivity) and in the fused one."""
    if which == "tunable_bus":
        Nt, nseeds = 21, B
        prob, u, pen = _case("tunable_bus", Nt)
    else:
        Nt, nseeds = 40, 2
        prob, u = _block_problem(NB=10, nblk=3, nu=2, m=2, Nt=Nt, seed=77)
        pen = ([0, 3, 5], [0], MU)
    pen = pen if with_pen else None
    N, m = prob.x0.shape
    W = np.random.default_rng(5).uniform(0.05, 0.4, size=(N, m))
    ref = [_source_reference(prob, u[b], W, pen) for b in range(nseeds)]
    src = np.stack([np.stack([2 * W * x for x in ref[b][2].x]) for b in range(nseeds)])
    e = _engine(prob, nseeds, monkeypatch, pen=pen)
    Js = e.propagate(u)
    e.set_costate_source(src)
    gs = e.grape_sensitivity(u, 3)
    info = e.info()
    assert info["backward"] == "blocks_prop16" and info["split_forward"] == "blocks_prop16", info
    _assert_batch(Js, gs, ref, ("source split", which, with_pen))
    _assert_costates(e, ref[1][2], 1, (0, 1, Nt // 2, Nt), ("source split", which, with_pen))
    if which == "tunable_bus":  # the odd block's rows carry λ_k (the source's), though no state
        odd = _rows(["010", "100", "001"])
        assert np.abs(ref[1][2].lam[0][odd]).max() == 0.0 or np.abs(e.costate(0, seed=1)[odd]).max() > 0.0
    J, g = _eval(e, u, True)
    assert e.info()["backward"] == "blocks_prop16", e.info()
    _assert_batch(J, g, ref, ("source fused", which, with_pen))
    _assert_costates(e, ref[0][2], 0, (0, Nt), ("source fused", which, with_pen))
    # without the source again: the penalised (or plain) eval
    e.set_costate_source(None)
    J2, g2 = _eval(e, u, True)
    for b in range(nseeds):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3, penalty=pen)
        _assert_seed(J2[b], g2[b], J0, g0, ("source cleared", which, with_pen, b))
    e.close()


@pytest.mark.parametrize("which,Nt", [("tunable_bus", 21), ("tunable_bus_cz", 21)])
def test_matches_chebyshev_block_chains(built_lib, monkeypatch, which, Nt):
    """The default against QOC_BLKP_PEN=0 (the Chebyshev-action block chains, the second implementation)."""
    prob, u, pen = _case(which, Nt)
    e = _engine(prob, B, monkeypatch, pen=pen)
    J, g = _eval(e, u, True)
    assert e.info()["backward"] == "blocks_prop16"
    e.close()
    ec = _engine(prob, B, monkeypatch, pen=pen, env={"QOC_BLKP_PEN": "0"})
    Jc, gc = _eval(ec, u, True)
    assert ec.info()["backward"] != "blocks_prop16", ec.info()
    ec.close()
    for b in range(B):
        _assert_seed(J[b], g[b], Jc[b], gc[b], (which, "PEN=0", b))


def test_other_orders_take_the_chebyshev_backward(built_lib, monkeypatch):
    """Order 2 is not on the λ chains: the penalised forward chain, then the Chebyshev block chains' backward and the
    dense gradient on its states, fused and split; order 3 afterwards is back on the λ chains."""
    Nt = 21
    prob, u, pen = _case("tunable_bus", Nt)
    ref2 = [O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=2, penalty=pen) for b in range(B)]
    e = _engine(prob, B, monkeypatch, pen=pen)
    J, g = _eval(e, u, True, order=2)
    assert e.info()["backward"] != "blocks_prop16", e.info()
    _assert_batch(J, g, ref2, "order 2 fused")
    Js = e.propagate(u)
    gs = e.grape_sensitivity(u, 2)
    assert e.info()["backward"] != "blocks_prop16", e.info()
    _assert_batch(Js, gs, ref2, "order 2 split")
    J3, g3 = _eval(e, u, True)
    assert e.info()["backward"] == "blocks_prop16", e.info()
    _assert_batch(J3, g3, _oracle("tunable_bus", Nt), "order 3 again")
    e.close()


@pytest.mark.parametrize("which,form", [("tunable_bus", "pair"), ("tunable_bus", "single"), ("tunable_bus_cz", "stored")])
def test_same_bits_every_time(built_lib, monkeypatch, which, form):
    """No atomics, fixed summation orders: the same u gives the same bits, on one engine and on a fresh one, fused and
    split."""
    Nt = 21
    prob, u, pen = _case(which, Nt)
    out = []
    for _ in range(2):
        e = _engine(prob, B, monkeypatch, pen=pen, env=FORMS[form])
        for _ in range(2):
            out.append(_eval(e, u, True))
            out.append((e.propagate(u), e.grape_sensitivity(u, 3)))
        e.close()
    for J, g in out[2::2]:
        assert np.array_equal(J, out[0][0]) and np.array_equal(g, out[0][1])
    for J, g in out[3::2]:
        assert np.array_equal(J, out[1][0]) and np.array_equal(g, out[1][1])


def test_no_effective_penalty_keeps_unpenalised_bits(built_lib, monkeypatch):
    """μ = 0, or penalised rows only in a dead block (x_k is zero there): bit for bit the unpenalised eval, fused and
    split."""
    Nt = 21
    prob, u, pen = _case("tunable_bus", Nt)
    out = {}
    for tag, p in (("none", None), ("mu0", (pen[0], pen[1], 0.0)), ("dead", (_rows(["010", "100"]), [0], MU))):
        e = _engine(prob, B, monkeypatch, pen=p)
        J, g = _eval(e, u, True)
        assert e.info()["backward"] == "blocks_prop16", (tag, e.info())
        Js, gs = e.propagate(u), e.grape_sensitivity(u, 3)
        assert e.info()["backward"] == "blocks_prop16", (tag, e.info())
        e.close()
        out[tag] = (J, g, Js, gs)
    for tag in ("mu0", "dead"):
        for a, r in zip(out[tag], out["none"]):
            assert np.array_equal(a, r), tag
    ref = _oracle("tunable_bus", Nt, False)
    _assert_batch(out["dead"][0], out["dead"][1], ref, "dead rows")


@pytest.mark.parametrize("form", ["pair", "stored"])
def test_stale_u_split_form(built_lib, monkeypatch, form):
    """grape_sensitivity with another u than propagate's: QOC_ERR_STALE and dJdu unwritten (the penalised backward
    launches read the queued flag themselves); the right u afterwards gives the oracle's gradient."""
    import torch
    from qoc_amd import StaleCacheError
    Nt = 21
    prob, u, pen = _case("tunable_bus", Nt)
    e = _engine(prob, B, monkeypatch, pen=pen, env=FORMS[form])
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    u2 = ud.clone()
    u2[1, 5, 0] += 1e-3
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.full((B, Nt, 1), 7.0, dtype=torch.float64, device="cuda")
    e.propagate_device(ud.data_ptr(), Jd.data_ptr())
    with pytest.raises(StaleCacheError):
        e.grape_sensitivity_device(u2.data_ptr(), 3, gd.data_ptr())
    e.synchronize()
    assert bool((gd == 7.0).all())
    e.grape_sensitivity_device(ud.data_ptr(), 3, gd.data_ptr())
    e.synchronize()
    assert e.info()["backward"] == "blocks_prop16", e.info()
    ref = _oracle("tunable_bus", Nt)
    _assert_batch(Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1)), ref, ("after stale", form))
    e.close()
