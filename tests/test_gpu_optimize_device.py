"""GPU: the device-resident multi-start optimiser (csrc/qoc_opt.hpp, include/qoc.h qoc_opt_* and
qoc_minimize_spline_dev) against its host reference qoc_amd.optimize.minimize_ticks.

The device and the host run the same per-seed state machine and differ only in the rounding of their reductions
(wave butterfly against numpy sums), so on problems away from the rounding floor of f every decision agrees: the
per-seed eval and iteration counts are equal and the iterates agree far below the bars (c 1e-9, f 1e-12 relative for
the analytic problems; c 1e-8, f 1e-10, lam 1e-6 for zz, the existing spline test's bars).  "Relative" for f is taken
against max(|f|, |f(c0)|) of the seed: Rosenbrock ends at f ~ 1e-20, where f itself carries no relative digits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- analytic objectives, elementwise torch on the GPU (a seed's value does not depend on the batch) -----------------
def _rowsum(a):
    acc = a[:, 0]
    for i in range(1, a.shape[1]):
        acc = acc + a[:, i]
    return acc


def rosen(x):
    a, c = x[:, 0], x[:, 1]
    f = (1 - a) ** 2 + 100 * (c - a * a) ** 2
    return f, torch.stack([-2 * (1 - a) - 400 * a * (c - a * a), 200 * (c - a * a)], 1)


def quadratic(sel=slice(None)):
    """The bounded quadratic of tests/test_optimize.py (B = 6, n = 5), products and sums spelled out elementwise."""
    torch.manual_seed(0)
    B, n = 6, 5
    Q = torch.randn(B, n, n, dtype=torch.float64)
    Q = Q @ Q.transpose(1, 2) + n * torch.eye(n, dtype=torch.float64)
    b = torch.randn(B, n, dtype=torch.float64) * 3
    Q, b = Q[sel].to(DEV), b[sel].to(DEV)

    def fg(x):
        r = Q[:, :, 0] * x[:, 0:1]
        for j in range(1, n):
            r = r + Q[:, :, j] * x[:, j:j + 1]
        return 0.5 * _rowsum(x * r) - _rowsum(b * x), r - b
    return fg


def diagonal(n=70, B=3):
    torch.manual_seed(3)
    dg = torch.linspace(1, 25, n, dtype=torch.float64).to(DEV)
    tt = torch.randn(B, n, dtype=torch.float64).to(DEV)

    def fg(x):
        return 0.5 * (dg * (x - tt) ** 2).sum(1), dg * (x - tt)
    return fg


def ball(x):
    """A quadratic whose minimum lies outside the unit ball, +inf outside the ball: trials are rejected for not being
    finite and, with max_ls = 2, line searches fail."""
    k = torch.tensor([1.0, 4.0, 9.0], dtype=torch.float64, device=x.device)
    t = torch.tensor([1.6, 0.3, -0.2], dtype=torch.float64, device=x.device)
    f = 0.5 * _rowsum(k * (x - t) ** 2)
    f = torch.where(_rowsum(x * x) > 1.0, torch.full_like(f, float("inf")), f)
    return f, k * (x - t)


def run_device(fg, c0, ticks, **kw):
    """Ask / tell on torch's stream for a fixed number of ticks: no readback between the evals."""
    from qoc_amd.optimize import DeviceOptimizer
    B, n = c0.shape
    opt = DeviceOptimizer(B, n, device=0, **kw)
    opt.start(c0)
    xt = opt.trial
    for _ in range(ticks):
        f, g = fg(xt)
        opt.tell(f, g)
    res = opt.result()
    opt.close()
    return res


def compare(dev, ref, f0, c_tol=1e-9, f_rel=1e-12):
    assert dev.evals.tolist() == ref.evals.tolist()
    assert dev.iters.tolist() == ref.iters.tolist()
    assert dev.ls_fails.tolist() == ref.ls_fails.tolist()
    assert dev.converged.tolist() == ref.converged.tolist()
    assert bool(dev.done.all()) and dev.not_done == 0 and dev.ticks == ref.ticks
    dc = float((dev.c - ref.c).abs().max())
    scale = torch.maximum(ref.f.abs(), f0.abs())
    df = float(((dev.f - ref.f).abs() / scale).max())
    print(f"max |dc| = {dc:.3e}, max rel |df| = {df:.3e}, evals {dev.evals.tolist()}")
    assert dc <= c_tol and df <= f_rel


CASES = {
    "rosenbrock": (lambda: rosen, [[-1.2, 1.0], [0.0, 0.0], [2.0, 2.0], [-0.5, 2.5]], dict(max_iter=300)),
    # B = 6: one full workgroup of four seeds and a partial one
    "bounded_quadratic": (quadratic, np.zeros((6, 5)), dict(lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6)),
    # n = 70: a lane holds two variables
    "diagonal_n70": (diagonal, np.zeros((3, 70)), dict(lower=-1.0, upper=1.0, max_iter=60, gtol=1e-6)),
    "ball_failed_line_searches": (lambda: ball, [[0.0, 0.9, 0.0], [-0.9, 0.0, 0.3], [0.1, 0.1, 0.95], [0.0, 0.0, 0.0]],
                                  dict(max_iter=8, max_ls=2, gtol=1e-6)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ask_tell_matches_host_state_machine(built_lib, name):
    from qoc_amd.optimize import minimize_ticks
    mk, c0, kw = CASES[name]
    fg = mk()
    c0 = torch.tensor(np.asarray(c0), dtype=torch.float64, device=DEV)
    ref = minimize_ticks(fg, c0, **kw)
    assert ref.not_done == 0
    if name == "ball_failed_line_searches":
        assert int(ref.ls_fails.min()) >= 1 and int(ref.iters.min()) >= 1
    if name == "bounded_quadratic":
        assert len(set(ref.evals.tolist())) > 1  # the seeds finish at different ticks
    dev = run_device(fg, c0, ref.ticks + 2, **kw)  # two ticks more: finished seeds no longer change
    compare(dev, ref, fg(c0)[0])


def test_a_seed_does_not_depend_on_its_batch(built_lib):
    from qoc_amd.optimize import minimize_ticks
    kw = dict(lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6)
    c0 = torch.zeros(6, 5, dtype=torch.float64, device=DEV)
    ticks = minimize_ticks(quadratic(), c0, **kw).ticks
    full = run_device(quadratic(), c0, ticks, **kw)
    alone = run_device(quadratic(slice(2, 3)), c0[2:3].clone(), ticks, **kw)
    assert torch.equal(alone.c[0], full.c[2]) and torch.equal(alone.f[0], full.f[2])
    assert int(alone.evals[0]) == int(full.evals[2]) and bool(alone.done[0])


# ---- zz through the engine ---------------------------------------------------------------------------------------
def _zz_engine(B):
    from qoc_amd import GrapeEngine, systems
    prob = systems.zz_problem(60)
    Bs = systems.spline_matrix(10.0, 60, 8)
    ns = Bs.shape[1]
    rng = np.random.default_rng(1)
    c0 = np.concatenate([0.01 * np.ones((B, ns)), np.zeros((B, ns))], 1) + 0.01 * rng.standard_normal((B, 2 * ns))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    return e, Bs, c0


def _zz_compare(dev, ref):
    assert dev.evals.tolist() == ref.evals.tolist()
    assert dev.ticks == int(ref.evals.max()) == ref.ticks == dev.n_evals
    assert dev.not_done == 0 and bool(dev.done.all()) and dev.history == []
    d = {k: float((getattr(dev, k) - getattr(ref, k)).abs().max()) for k in ("c", "f", "lam")}
    print(f"max |dc| = {d['c']:.3e}, |df| = {d['f']:.3e}, |dlam| = {d['lam']:.3e}, evals {dev.evals.tolist()}")
    assert d["c"] <= 1e-8 and d["f"] <= 1e-10 and d["lam"] <= 1e-6
    assert torch.equal(dev.rho, ref.rho)
    assert dev.iters.tolist() == ref.iters.tolist() and dev.rounds.tolist() == ref.rounds.tolist()


def test_zz_reference_bounds_against_host_machine_and_lockstep(built_lib):
    from qoc_amd.optimize import SplineGrape, minimize_batched, minimize_on_device, minimize_ticks
    e, Bs, c0 = _zz_engine(3)
    bound = 2 * np.pi * 0.060
    kw = dict(lower=-bound, upper=bound, g_upper=[2.0, 1.0], max_iter=12, outer_iters=1)
    sg = SplineGrape(e, Bs)
    c0d = torch.from_numpy(c0).to(DEV)
    ref = minimize_ticks(sg.fg, c0d, cons=sg.cons, **kw)
    lock = minimize_batched(sg.fg, c0d, cons=sg.cons, **kw)
    dev = minimize_on_device(e, Bs, c0d, **kw)
    _zz_compare(dev, ref)
    assert int(dev.evals.max()) <= lock.n_evals
    np.testing.assert_allclose(dev.c.cpu().numpy(), lock.c.cpu().numpy(), rtol=0, atol=1e-8)
    np.testing.assert_allclose(dev.f.cpu().numpy(), lock.f.cpu().numpy(), rtol=0, atol=1e-10)
    e.close()


ZZ2 = dict(lower=-0.2, upper=0.2, g_upper=[0.6, 0.3], max_iter=6, outer_iters=3, rho0=10.0)


@pytest.fixture(scope="module")
def zz_constrained(built_lib):
    """Setting (ii): tight bounds, the norm constraint active, three rounds with the penalty raised, uneven per-seed
    counts.  One fused run, its host reference, and the same run unfused, on one engine."""
    from qoc_amd.optimize import DeviceOptimizer, SplineGrape, minimize_on_device, minimize_ticks
    B = 5
    e, Bs, c0 = _zz_engine(B)
    ns, nu = Bs.shape[1], 2
    sg = SplineGrape(e, Bs)
    c0d = torch.from_numpy(c0).to(DEV)
    ref = minimize_ticks(sg.fg, c0d, cons=sg.cons, **ZZ2)
    dev = minimize_on_device(e, Bs, c0d, **ZZ2)
    best = e.allgather_best()  # of the closing eval
    J_again = e.eval_spline(dev.c.cpu().numpy().reshape(B, nu, ns).transpose(0, 2, 1))[0]
    # unfused: eval_spline_device at the trials, then the generic tell kernel (the same opt_tell; it computes the norm
    # constraints itself), everything on the engine's stream
    opt = DeviceOptimizer(B, ns * nu, ns=ns, nu=nu, device=0, stream=e.stream(), **ZZ2)
    J = torch.empty(B, dtype=torch.float64, device=DEV)
    G = torch.empty(B, ns * nu, dtype=torch.float64, device=DEV)
    gv = torch.empty(B, 2, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    opt.start(c0d)
    for _ in range(dev.ticks):
        e.eval_spline_device(opt.trial_ptr(), 3, J.data_ptr(), G.data_ptr())
        opt.tell(J.data_ptr(), G.data_ptr())
    unfused = opt.result()
    from qoc_amd import _lib
    e.spline_constraints_device(opt.field_ptr(_lib.QOC_OPT_X), gv.data_ptr())
    e.synchronize()
    opt.close()
    out = dict(ref=ref, dev=dev, best=best, J_again=J_again, unfused=unfused, g_kernel=gv.cpu())
    e.close()
    return out


def test_zz_constrained_against_host_machine(zz_constrained):
    dev, ref = zz_constrained["dev"], zz_constrained["ref"]
    _zz_compare(dev, ref)
    assert dev.rounds.tolist() == [3] * 5
    assert len(set(dev.evals.tolist())) > 1            # uneven per-seed counts
    assert float(dev.lam.max()) > 0 and float(dev.rho.max()) > 10.0   # a constraint is active, the penalty was raised
    assert float(dev.c.abs().max()) <= 0.2 and int((dev.c.abs() == 0.2).sum()) > 0  # coefficients on a bound


def test_fused_step_is_the_unfused_run(zz_constrained):
    dev, unf = zz_constrained["dev"], zz_constrained["unfused"]
    assert torch.equal(dev.c, unf.c) and torch.equal(dev.f, unf.f)
    assert torch.equal(dev.lam, unf.lam) and dev.evals.tolist() == unf.evals.tolist()
    # the constraints the state machine computes in its wave against k_spline_constraints
    np.testing.assert_allclose(dev.g.cpu().numpy(), zz_constrained["g_kernel"].numpy(), rtol=1e-14, atol=0)


def test_closing_eval_and_best_seed(zz_constrained):
    dev = zz_constrained["dev"]
    f = dev.f.cpu().numpy()
    # f was evaluated on the fused step's u = Bs c; eval_spline maps the same c with k_spline_u
    assert np.array_equal(f, zz_constrained["J_again"])
    Jb, sb = zz_constrained["best"]
    assert Jb == f.min() and sb == int(f.argmin())


def test_errors(built_lib):
    from qoc_amd import GrapeEngine, QOCError, _lib, systems
    from qoc_amd.optimize import DeviceOptimizer
    for kw in (dict(n=257), dict(n=8, memory=17)):
        with pytest.raises(QOCError) as ei:
            DeviceOptimizer(2, **kw)
        assert ei.value.code == _lib.QOC_ERR_UNSUPPORTED
    prob = systems.zz_problem(20)
    Bs = systems.spline_matrix(10.0, 20, 4)
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=2)
    e.set_cost_trace(prob.x_target, prob.n)
    c = torch.zeros(2, 8, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()

    def attempt(B, ns, code):
        opt = DeviceOptimizer(B, ns * 2, ns=ns, nu=2, g_upper=[2.0, 1.0], max_iter=3, device=0, stream=e.stream())
        with pytest.raises(QOCError) as ei:
            e.minimize_spline_device(opt, c.data_ptr(), 10)
        assert ei.value.code == code
        opt.close()
    attempt(2, 4, _lib.QOC_ERR_STATE)  # no spline basis
    e.set_spline_basis(Bs)
    attempt(3, 4, _lib.QOC_ERR_ARG)    # another B
    attempt(2, 3, _lib.QOC_ERR_ARG)    # another n
    e.close()
