"""The guard-state penalty (setup_state_penalty, src/penalty_fcns.jl:1-11; consumed at
src/gradient_computations.jl:47-49,55-57) on the segmented block eval (csrc/qoc_blkseg.hpp, the PEN instantiations):
L(x_k) = μ Σ_{i in P, c in C} |x_k[i, c]|^2 summed over the Nt + 1 states in J, and the source 2 μ x_k[P, C] of λ_k
carried as D_k = Σ_{c in C} x_k,c x_k,c^H beside G_k, so that no state goes to HBM.

Against oracle/qoc_oracle.grape_eval(..., penalty=...) at the fp64 bar of SURVEY.md §8c: |ΔJ| <= 1e-12 and
||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed; states and co-states (rebuilt on demand) 1e-12 relative to the trajectory's
largest entry.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import MU, assert_seed as _assert_seed, block_problem as _block_problem, case as _case
from blkseg_util import bufs as _bufs, dev as _dev, engine as _engine, eval_dev as _eval_dev, pen as _pen
from blkseg_util import split_dev as _split_dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(name, order=3):
    """The oracle's (J, dJdu, cache) of every seed of a shipped case: computed once, shared, never changed."""
    prob, u, pen = _case(name)
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=order, penalty=_pen(pen))
                 for b in range(u.shape[0]))


def _block_penalty(blocks, m):
    """Every row of one block, one row of another, a row of the short last block (the other blocks have none); a
    strict subset of the columns (a single one for m = 2, 3), m = 1: its only column."""
    P = list(blocks[1]) + [blocks[3][-1]] + [blocks[-1][0]]
    C = [0] if m == 1 else [1] if m <= 3 else [0, 2]
    return P, C, MU


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_penalised_eval_matches_oracle_states_costates(built_lib, monkeypatch, name):
    """J (with the penalty's sum over all Nt + 1 states) and dJdu on the segmented path; x_k and λ_k (with the source
    of every slice, λ_0 the one of k = 0 included) rebuilt on demand."""
    prob, u, pen = _case(name)
    B = u.shape[0]
    e = _engine(prob, B, monkeypatch, pen=_pen(pen))
    J, g = _eval_dev(e, u)
    info = e.info()
    assert info["backward"] == "segmented" and info["chain_kernel"] == "blocks_prop", info
    ks = (0, 1, prob.Nt // 2, prob.Nt - 1, prob.Nt)
    xs = [e.state(k, seed=B - 1) for k in ks]
    lams = [e.costate(k, seed=B - 1) for k in ks]
    e.close()
    ref = _oracle(name)
    for b in range(B):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, b))
    c0 = ref[B - 1][2]
    xsc = max(np.abs(x).max() for x in c0.x)
    lsc = max(np.abs(lam).max() for lam in c0.lam)
    for k, x, lam in zip(ks, xs, lams):
        assert np.abs(x - c0.x[k]).max() <= 1e-12 * xsc, ("x", k)
        assert np.abs(lam - c0.lam[k]).max() <= 1e-12 * lsc, ("lambda", k)


@pytest.mark.parametrize("S", [1, 2, 7, 13, None])
@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_penalised_segment_counts(built_lib, monkeypatch, name, S):
    """One segment (no scan, no suffix sum), ragged last segments, one slice per segment (S = Nt)."""
    prob, u, pen = _case(name)
    e = _engine(prob, u.shape[0], monkeypatch, pen=_pen(pen), S=prob.Nt if S is None else S)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    ref = _oracle(name)
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, S, b))


@pytest.mark.parametrize("W", [1, 3, 8])
def test_penalised_waves_per_seed(built_lib, monkeypatch, W):
    """1, 3 or 8 waves per seed on cavity N = 40, Nt = 77: the suffix sums within one wave and over the waves' totals."""
    prob, u, pen = _case("cavity40")
    e = _engine(prob, u.shape[0], monkeypatch, pen=_pen(pen), W=W)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    ref = _oracle("cavity40")
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (W, b))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_penalised_gradient_orders(built_lib, monkeypatch, name, order):
    prob, u, pen = _case(name)
    e = _engine(prob, u.shape[0], monkeypatch, pen=_pen(pen))
    J, g = _eval_dev(e, u, order)
    assert e.info()["backward"] == "segmented"
    e.close()
    ref = _oracle(name, order)
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, order, b))


@pytest.mark.parametrize("NB,nblk,nu,m", [(2, 7, 1, 3), (2, 24, 2, 1), (3, 5, 2, 2), (3, 9, 1, 4)])
def test_penalised_random_permuted_blocks(built_lib, monkeypatch, NB, nblk, nu, m):
    """Random permuted blocks (the general Taylor path, padding lanes): blocks with all, one and no penalised row, a
    penalised row in the short block, a strict subset of the columns."""
    prob, u, blocks = _block_problem(NB, nblk, nu, m, Nt=45, seed=NB * 100 + nblk + nu + m)
    pen = _block_penalty(blocks, m)
    e = _engine(prob, 2, monkeypatch, pen=pen)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    lam = e.costate(0, seed=1)
    e.close()
    for b in range(2):
        J0, g0, c0 = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3, penalty=pen)
        _assert_seed(J[b], g[b], J0, g0, (NB, nblk, nu, m, b))
    lsc = max(np.abs(v).max() for v in c0.lam)
    assert np.abs(lam - c0.lam[0]).max() <= 1e-12 * lsc


def test_penalised_zcalibrated_cost(built_lib, monkeypatch):
    """The z-calibrated cost with the penalty on zz: J against the oracle's cost of its own x_N plus the penalty's
    sum; the gradient less the penalty's own part (linear in the source; the oracle's, with a zero final cost) against
    the oracle's family g(Δθ) within the calibration phase's bound, as tests/test_gpu_blkseg.py holds it."""
    from qoc_amd import systems
    prob = systems.zz_problem(40, tgate=4.0)
    u = systems.zz_controls(2, 40, 4.0, seed=86)
    qb = systems.QuantumBasis([3, 3])
    pen = ([int(r) for r in qb(["20", "21", "22"])], [0, 1, 2, 3], MU)
    Jz, _ = O.setup_infidelity_zcalibrated(prob.x_target)
    Lf, _ = O.setup_state_penalty(*pen)
    e = _engine(prob, 2, monkeypatch, pen=pen)
    e.set_cost_zcalibrated(prob.x_target)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    zero = (lambda x: 0.0, lambda x: np.zeros_like(np.asarray(x, dtype=complex)))
    for b in range(2):
        xs = O.propagate(prob.A0, prob.A, u[b], prob.x0)
        assert abs(J[b] - (Jz(xs[-1]) + sum(Lf(x) for x in xs))) <= 1e-12
        gpen = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=3, penalty=pen, cost=zero)[1]
        res, dth = O.zcal_gradient_match(g[b] - gpen, prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=3)
        assert res <= 1e-10 and abs(dth) <= O.zcal_dtheta_bound(prob.x_target, xs[-1]), (b, res, dth)


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_penalised_split_form(built_lib, monkeypatch, name):
    """propagate then grape_sensitivity (the reference's f / f_grad) with the penalty: both halves segmented, J and
    dJdu bitwise the fused eval's, a different u refused with nothing written."""
    from qoc_amd import StaleCacheError
    prob, u, pen = _case(name)
    B, nu, Nt = u.shape
    e = _engine(prob, B, monkeypatch, pen=_pen(pen))
    J, g = _split_dev(e, u)
    info = e.info()
    assert info["split_forward"] == "segmented" and info["backward"] == "segmented", info
    Jf, gf = _eval_dev(e, u)
    assert np.array_equal(J, Jf) and np.array_equal(g, gf)
    u2 = u.copy()
    u2[1, 0, Nt // 3] += 1e-9
    ud, ud2 = _dev(u), _dev(u2)
    Jd, gd = _bufs(B, Nt, nu)
    e.propagate_device(ud.data_ptr(), Jd.data_ptr())
    with pytest.raises(StaleCacheError):
        e.grape_sensitivity_device(ud2.data_ptr(), 3, gd.data_ptr())
    e.synchronize()
    assert np.all(np.isnan(gd.cpu().numpy()))
    e.close()
    ref = _oracle(name)
    for b in range(B):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, b))


def test_penalised_per_seed_x0(built_lib, monkeypatch):
    """A distinct x_0 per seed: D_0 is the seed's own."""
    prob, u, pen = _case("cavity20")
    pen = _pen(pen)
    rng = np.random.default_rng(7)
    x0s = np.stack([np.linalg.qr(rng.standard_normal(prob.x0.shape) + 1j * rng.standard_normal(prob.x0.shape))[0]
                    for _ in range(3)])
    e = _engine(prob, 3, monkeypatch, pen=pen)
    e.set_x0(x0s, per_seed=True)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    for b in range(3):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], x0s[b], prob.x_target, prob.n, order=3, penalty=pen)
        _assert_seed(J[b], g[b], J0, g0, ("x0", b))


def test_penalty_retargeted_on_one_context(built_lib, monkeypatch):
    """One context: a penalised eval; the penalty cleared (bitwise a fresh unpenalised context's result); another
    (P, C, μ); then generators with another block layout (N = 17: 9 blocks of 2 rows, then 6 blocks of 3), for which
    the rows' masks are derived anew."""
    pa, u, ba = _block_problem(2, 9, 2, 2, Nt=45, seed=31)
    pb, _, bb = _block_problem(3, 6, 2, 2, Nt=45, seed=32)
    pen1 = (list(ba[0]) + [ba[4][0]], [1], MU)
    pen2 = ([ba[2][1], ba[-1][0], ba[5][0]], [0, 1], 0.21)
    e = _engine(pa, 2, monkeypatch, pen=pen1)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    for b in range(2):
        J0, g0, _ = O.grape_eval(pa.A0, pa.A, u[b], pa.x0, pa.x_target, pa.n, order=3, penalty=pen1)
        _assert_seed(J[b], g[b], J0, g0, ("pen1", b))
    e.set_state_penalty([], [], 0.0)
    Jn, gn = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.set_state_penalty(*pen2)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    for b in range(2):
        J0, g0, _ = O.grape_eval(pa.A0, pa.A, u[b], pa.x0, pa.x_target, pa.n, order=3, penalty=pen2)
        _assert_seed(J[b], g[b], J0, g0, ("pen2", b))
    e.set_generators(pb.A0, pb.A)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    for b in range(2):
        J0, g0, _ = O.grape_eval(pb.A0, pb.A, u[b], pa.x0, pa.x_target, pa.n, order=3, penalty=pen2)
        _assert_seed(J[b], g[b], J0, g0, ("layout", b))
    e = _engine(pa, 2, monkeypatch)
    J0, g0 = _eval_dev(e, u)
    e.close()
    assert np.array_equal(Jn, J0) and np.array_equal(gn, g0)


def test_penalised_fallbacks_stay(built_lib, monkeypatch):
    """A co-state source keeps the block chains (an arbitrary dL/dx needs x_k), the penalty included in both J and
    λ_k; QOC_BLKSEG_PEN=0 keeps a penalised eval off the segmented path, and both paths agree to the bars."""
    prob, u, pen = _case("zz")
    pen = _pen(pen)
    B = u.shape[0]
    ref = _oracle("zz")
    # the source: dL/dx of a second penalty at the engine's own states; its gradient adds to the first one's
    pen2 = ([3, 4], [1, 2], 0.11)
    _, dL2 = O.setup_state_penalty(*pen2)
    zero = (lambda x: 0.0, lambda x: np.zeros_like(np.asarray(x, dtype=complex)))
    e = _engine(prob, B, monkeypatch, pen=pen)
    e.propagate(u)
    src = np.stack([np.stack([dL2(e.state(k, seed=b)) for k in range(prob.Nt + 1)]) for b in range(B)])
    e.set_costate_source(src)
    J = e.propagate(u)
    g = e.grape_sensitivity(u, 3)
    assert e.info()["backward"] != "segmented", e.info()
    e.close()
    for b in range(B):
        g2 = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3, penalty=pen2, cost=zero)[1]
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1] + g2, ("source", b))
    out = {}
    for sw in ("0", None):
        e = _engine(prob, B, monkeypatch, pen=pen, segpen=sw)
        out[sw] = _eval_dev(e, u) + (e.info()["backward"],)
        e.close()
    assert out["0"][2] != "segmented" and out[None][2] == "segmented", (out["0"][2], out[None][2])
    for b in range(B):
        _assert_seed(out["0"][0][b], out["0"][1][b], ref[b][0], ref[b][1], ("switch off", b))
        _assert_seed(out[None][0][b], out[None][1][b], out["0"][0][b], out["0"][1][b], ("paths", b))


def test_penalised_best_pair(built_lib, monkeypatch):
    """The launch's best (J, seed) is taken from the penalised J."""
    from qoc_amd import systems
    prob = systems.cavity_problem(N_cavity=10, Nt=24)
    B = 300
    u = systems.cavity_controls(B, prob.Nt, seed=91) * 6.0  # spread the fidelities
    pen = ([16, 17, 18, 19, 5], [0, 1], MU)
    e = _engine(prob, B, monkeypatch, pen=pen)
    J, _ = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    best = e.allgather_best()
    e.close()
    e = _engine(prob, B, monkeypatch)
    Jn, _ = _eval_dev(e, u)
    e.close()
    assert best == (J.min(), int(np.argmin(J)))
    b = int(np.argmin(J))
    Jr = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3, penalty=pen)[0]
    assert abs(J[b] - Jr) <= 1e-12 and np.all(J > Jn)
