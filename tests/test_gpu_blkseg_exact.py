"""The exact (Fréchet) gradient on the segmented block eval (csrc/qoc_blkseg.hpp, the ORD 0 instantiations of
k_blkseg_eval): dUkdp_order = "exact" stays on the one-launch eval of the generators with invariant blocks of <= 3 rows
(cavity: blocks of 2, zz: blocks of 3), with the contraction Re tr(A_j M(K_k)) taken over the whole series
M = Σ_{a,b} X^b K X^a / (a+b+1)! (closed form on blocks of 2 rows without halvings; the series to the seed's term
count otherwise).

The bar is the project's fp64 bar against oracle/qoc_oracle.grape_eval(..., order="exact"):
|ΔJ| <= 1e-12 and ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed; states and co-states (rebuilt on demand) 1e-12 relative to the
trajectory's largest entry.  The oracle's own exact gradient lies 7e-6 (zz) to 4e-5 (cavity) away from its order 3 on
these cases, so an eval that ran order 3 under the exact tag would miss the bar by five orders.

The recipes (_engine, _eval_dev, _split_dev, _block_problem, the shipped cases and their penalties) are those of
tests/blkseg_util.py.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import MU, assert_seed as _assert_seed, block_problem as _block_problem, case as _case
from blkseg_util import bufs as _bufs, dev as _dev, engine as _engine, eval_dev, pen as _pen, split_dev

pytestmark = pytest.mark.gpu

EX = "exact"


def _eval_dev(e, u, order=EX):
    return eval_dev(e, u, order)


def _split_dev(e, u, order=EX, check=None):
    return split_dev(e, u, order, check)


@functools.lru_cache(maxsize=None)
def _oracle(name, order=EX, pen=False):
    """The oracle's (J, dJdu, cache) of every seed of a shipped case: computed once, shared, never changed."""
    prob, u, p = _case(name)
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=order,
                              penalty=_pen(p) if pen else None) for b in range(u.shape[0]))


def _theta(P):
    """θ_P: the largest β with Σ_{t > P} β^t / t! <= 2^-53 (the engine's Taylor-tail thresholds; θ_17 ≈ 0.98 caps the
    scaled slice, beyond it the kernel halves)."""
    def tail(b):
        term, s = 1.0, 0.0
        for t in range(1, P + 60):
            term *= b / t
            if t > P:
                s += term
        return s
    lo, hi = 0.0, 64.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tail(mid) <= 2.0 ** -53 else (lo, mid)
    return lo


def _rho_lower(prob, u):
    """A lower bound of the seeds' largest ρ_k = rad_0 + Σ_j |u_jk| rad_j: the spectral half-width of each generator
    (no scalar shift leaves a smaller radius)."""
    rad = []
    for A in [prob.A0] + list(prob.A):
        ev = np.linalg.eigvalsh(1j * np.asarray(A))
        rad.append(0.5 * (ev[-1] - ev[0]))
    return max(rad[0] + sum(abs(u[b, j, k]) * rad[j + 1] for j in range(u.shape[1]))
               for b in range(u.shape[0]) for k in range(u.shape[2]))


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_exact_eval_stays_segmented_and_matches_oracle(built_lib, monkeypatch, name):
    """eval_device(..., "exact") stays on the segmented path (the parent left it for the dense Fréchet kernel) and
    meets the oracle's exact J and dJdu; x_k and λ_k, rebuilt on demand, meet the oracle's trajectories."""
    prob, u, _ = _case(name)
    B = u.shape[0]
    e = _engine(prob, B, monkeypatch)
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
    # the cases tell the two gradients apart: the oracle's order 3 is far outside the bar
    g3 = _oracle(name, 3)[0][1]
    assert np.linalg.norm(g3 - ref[0][1]) / np.linalg.norm(ref[0][1]) > 1e-7
    c0 = ref[B - 1][2]
    xsc = max(np.abs(x).max() for x in c0.x)
    lsc = max(np.abs(lam).max() for lam in c0.lam)
    for k, x, lam in zip(ks, xs, lams):
        assert np.abs(x - c0.x[k]).max() <= 1e-12 * xsc, ("x", k)
        assert np.abs(lam - c0.lam[k]).max() <= 1e-12 * lsc, ("lambda", k)


@pytest.mark.parametrize("S", [1, 7, 50])
@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_exact_segment_counts(built_lib, monkeypatch, name, S):
    """One segment (no scan), a ragged last segment, one slice per segment (cavity20: S = Nt)."""
    prob, u, _ = _case(name)
    e = _engine(prob, u.shape[0], monkeypatch, S=S)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    ref = _oracle(name)
    for b in range(u.shape[0]):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, S, b))


@pytest.mark.parametrize("amp", [1.0, 8.0, 14.0, 22.0])
def test_exact_series_degree_classes_and_halving(built_lib, monkeypatch, amp):
    """Blocks of 2 rows: the closed form's series (cos, sinc and s3) at K = 5 / 7 / 9 (ρ <= 0.24 / 0.66 / θ_cap); amp = 22
    exceeds θ_cap, where blocks of 2 rows take the generic series (ρ ≈ 1.25: about 20 orders)."""
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=40)
    u = systems.cavity_controls(3, p.Nt, seed=91) * amp
    if amp == 22.0:
        assert _rho_lower(p, u) > _theta(17)
    e = _engine(p, 3, monkeypatch)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented"
    e.close()
    for b in range(3):
        J0, g0, _ = O.grape_eval(p.A0, p.A, u[b], p.x0, p.x_target, p.n, order=EX)
        _assert_seed(J[b], g[b], J0, g0, (amp, b))


@pytest.mark.parametrize("NB,nblk,nu,m,scale", [(2, 7, 1, 3, 1.0), (2, 24, 2, 1, 1.0), (3, 5, 2, 2, 1.0),
                                                (3, 9, 1, 4, 1.0), (3, 5, 2, 2, 5.0)])
def test_exact_random_permuted_blocks(built_lib, monkeypatch, NB, nblk, nu, m, scale):
    """Random permuted blocks of 2 / 3 rows (padding rows, one control, two segments per wave); the last case raises
    the generators so that blocks of 3 rows run with halvings (J > 0: ρ beyond θ_17, checked here on the CPU)."""
    prob, u, _ = _block_problem(NB, nblk, nu, m, Nt=45, seed=NB * 100 + nblk + nu + m, scale=scale)
    if scale != 1.0:
        assert _rho_lower(prob, u) > _theta(17)
    e = _engine(prob, 2, monkeypatch)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    for b in range(2):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=EX)
        _assert_seed(J[b], g[b], J0, g0, (NB, nblk, nu, m, scale, b))


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_exact_with_the_guard_state_penalty(built_lib, monkeypatch, name):
    """The penalised exact eval, fused and as propagate + grape_sensitivity: both stay segmented (zz: the fused call is
    the forward and the backward half), bitwise the same, at the bar against the oracle's penalised exact gradient."""
    prob, u, pen = _case(name)
    B = u.shape[0]
    e = _engine(prob, B, monkeypatch, pen=_pen(pen))
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    Js, gs = _split_dev(e, u)
    info = e.info()
    assert info["split_forward"] == "segmented" and info["backward"] == "segmented", info
    e.close()
    assert np.array_equal(J, Js) and np.array_equal(g, gs)
    ref = _oracle(name, pen=True)
    for b in range(B):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, b))


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_exact_split_form(built_lib, monkeypatch, name):
    """propagate then grape_sensitivity(u, "exact"): the forward half is segmented before the backward runs and the
    backward after it; dJdu is bitwise the fused exact eval's, J bitwise an order-3 eval's (the forward has no order);
    a changed u is refused with nothing written."""
    from qoc_amd import StaleCacheError
    prob, u, _ = _case(name)
    B, nu, Nt = u.shape
    e = _engine(prob, B, monkeypatch)
    seen = {}
    J, g = _split_dev(e, u, check=lambda info: seen.update(info))
    assert seen["split_forward"] == "segmented", seen
    assert e.info()["backward"] == "segmented" and e.info()["split_forward"] == "segmented", e.info()
    Jf, gf = _eval_dev(e, u)
    J3, _ = _eval_dev(e, u, 3)
    assert np.array_equal(g, gf) and np.array_equal(J, Jf) and np.array_equal(J, J3)
    u2 = u.copy()
    u2[1, 0, Nt // 3] += 1e-9
    ud, ud2 = _dev(u), _dev(u2)
    Jd, gd = _bufs(B, Nt, nu)
    e.propagate_device(ud.data_ptr(), Jd.data_ptr())
    with pytest.raises(StaleCacheError):
        e.grape_sensitivity_device(ud2.data_ptr(), EX, gd.data_ptr())
    e.synchronize()
    assert np.all(np.isnan(gd.cpu().numpy()))
    e.close()
    ref = _oracle(name)
    for b in range(B):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], (name, b))


@pytest.mark.parametrize("name", ["zz", "cavity20"])
def test_exact_switch_keeps_the_dense_frechet_path(built_lib, monkeypatch, name):
    """QOC_BLKSEG_EXACT=0: the same inputs leave the segmented path (x_k and λ_k rebuilt, the dense Fréchet kernel); the
    two implementations agree to the bar, and orders 1..4 do not read the switch."""
    prob, u, _ = _case(name)
    B = u.shape[0]
    out = {}
    for sw in ("0", None):
        e = _engine(prob, B, monkeypatch, segex=sw)
        out[sw] = _eval_dev(e, u) + (e.info()["backward"],)
        if sw == "0":
            _eval_dev(e, u, 3)
            assert e.info()["backward"] == "segmented"
        e.close()
    assert out["0"][2] != "segmented" and out[None][2] == "segmented", (out["0"][2], out[None][2])
    for b in range(B):
        _assert_seed(out[None][0][b], out[None][1][b], out["0"][0][b], out["0"][1][b], (name, "paths", b))


def test_exact_zcalibrated_cost_against_the_dense_path(built_lib, monkeypatch):
    """The z-calibrated cost on zz (Nt = 40, B = 2): the segmented exact eval against the dense Fréchet path
    (QOC_BLKSEG_EXACT=0) on the same inputs, J against the oracle's cost of its own x_N."""
    from qoc_amd import systems
    prob = systems.zz_problem(40, tgate=4.0)
    u = systems.zz_controls(2, 40, 4.0, seed=86)
    Jz, _ = O.setup_infidelity_zcalibrated(prob.x_target)
    out = {}
    for sw in ("0", None):
        e = _engine(prob, 2, monkeypatch, segex=sw)
        e.set_cost_zcalibrated(prob.x_target)
        out[sw] = _eval_dev(e, u) + (e.info()["backward"],)
        e.close()
    assert out["0"][2] != "segmented" and out[None][2] == "segmented", (out["0"][2], out[None][2])
    for b in range(2):
        xN = O.propagate(prob.A0, prob.A, u[b], prob.x0)[-1]
        assert abs(out[None][0][b] - Jz(xN)) <= 1e-12
        _assert_seed(out[None][0][b], out[None][1][b], out["0"][0][b], out["0"][1][b], ("zcal", b))


@pytest.mark.parametrize("amp", [1.0, 22.0])
def test_exact_is_the_derivative_of_the_computed_cost(built_lib, monkeypatch, amp):
    """cavity20: central differences of the device's own J along one random direction d (h = 1e-6) against g·d.  The
    exact gradient meets them to 1e-6 relative; order 3 at controls x 22 does not (it is off by about a factor of two
    there), which is why the mode exists."""
    prob, u, _ = _case("cavity20")
    u = u[:1] * amp
    rng = np.random.default_rng(5)
    d = rng.standard_normal(u.shape)
    d /= np.linalg.norm(d)
    h = 1e-6
    e = _engine(prob, 3, monkeypatch)
    J, g = _eval_dev(e, np.concatenate([u, u + h * d, u - h * d]))
    assert e.info()["backward"] == "segmented"
    _, g3 = _eval_dev(e, np.concatenate([u, u, u]), 3)
    e.close()
    fd = (J[1] - J[2]) / (2 * h)
    dex, d3 = float(np.sum(g[0] * d[0])), float(np.sum(g3[0] * d[0]))
    print(f"amp {amp}: fd {fd:.10e} exact {dex:.10e} order 3 {d3:.10e}")
    assert abs(dex - fd) <= 1e-6 * abs(fd), (amp, dex, fd)
    if amp == 22.0:
        assert abs(d3 - fd) > 1e-6 * abs(fd), (amp, d3, fd)


def test_exact_device_optimiser_on_the_segmented_eval(built_lib, monkeypatch):
    """The setting of tests/test_gpu_optimize_device.py's zz run (reference bounds, B = 3) at order "exact": the
    device-resident optimiser against the host state machine driven by SplineGrape(order="exact"), with that test's
    checks; the evals behind both are the segmented kernel's."""
    import torch
    from qoc_amd import GrapeEngine, systems
    from qoc_amd.optimize import SplineGrape, minimize_on_device, minimize_ticks
    for k in ("QOC_BLKSEG", "QOC_BLKSEG_EXACT", "QOC_BLKSEG_S", "QOC_BLKSEG_W", "QOC_BLOCKS", "QOC_BLKU"):
        monkeypatch.delenv(k, raising=False)
    B = 3
    prob = systems.zz_problem(60)
    Bs = systems.spline_matrix(10.0, 60, 8)
    ns = Bs.shape[1]
    rng = np.random.default_rng(1)
    c0 = np.concatenate([0.01 * np.ones((B, ns)), np.zeros((B, ns))], 1) + 0.01 * rng.standard_normal((B, 2 * ns))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    bound = 2 * np.pi * 0.060
    kw = dict(lower=-bound, upper=bound, g_upper=[2.0, 1.0], max_iter=12, outer_iters=1)
    sg = SplineGrape(e, Bs, order=EX)
    c0d = torch.from_numpy(c0).to("cuda:0")
    ref = minimize_ticks(sg.fg, c0d, cons=sg.cons, **kw)
    assert e.info()["backward"] == "segmented", e.info()
    dev = minimize_on_device(e, Bs, c0d, order=EX, **kw)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    assert dev.evals.tolist() == ref.evals.tolist()
    assert dev.ticks == int(ref.evals.max()) == ref.ticks == dev.n_evals
    assert dev.not_done == 0 and bool(dev.done.all()) and dev.history == []
    d = {k: float((getattr(dev, k) - getattr(ref, k)).abs().max()) for k in ("c", "f", "lam")}
    print(f"max |dc| = {d['c']:.3e}, |df| = {d['f']:.3e}, |dlam| = {d['lam']:.3e}, evals {dev.evals.tolist()}")
    assert d["c"] <= 1e-8 and d["f"] <= 1e-10 and d["lam"] <= 1e-6
    assert torch.equal(dev.rho, ref.rho)
    assert dev.iters.tolist() == ref.iters.tolist() and dev.rounds.tolist() == ref.rounds.tolist()
