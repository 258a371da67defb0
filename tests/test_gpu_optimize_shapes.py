"""GPU: the device optimiser (csrc/qoc_opt.hpp opt_tell, k_opt_step_spline) and the host loop of
qoc_minimize_spline_dev at the shapes where their index arithmetic changes: every register row of a lane, the row
boundaries, the constraint differences across lanes and rows, the history ring at memory 1, 2 and 16, the curvature
skip, the second pass of the fused step's gradient and control-writing loops, lanes without a slice, nu = 1, and
max_ticks / poll_every.

The reference is the host machine qoc_amd.optimize.minimize_ticks on the same f and g (tests/opt_cases.py); that its
decisions do not hinge on the order of a sum is checked on the CPU by tests/test_optimize_cases_algebra.py.  Bars are
those of tests/test_gpu_optimize_device.py, unchanged: equal counts, |dc| <= 1e-9 and |df| <= 1e-12 relative to
max(|f|, |f(c0)|) for the analytic cases (|dlam| <= 1e-6 and equal rho with constraints); _zz_compare's for the engine
cases (|dc| <= 1e-8, |df| <= 1e-10, |dlam| <= 1e-6).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import opt_cases as OC
from test_gpu_optimize_device import ZZ2, _zz_compare, compare, run_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- A. ask / tell against the host machine ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.BY_NAME))
def test_ask_tell_shapes_match_host_state_machine(built_lib, name):
    """Every case of tests/opt_cases.py: rows 2 and 3 of the lane registers and the boundaries n = 64/65, 128/129,
    192/193, 256 (dots, two-loop recursion, free set, clamp); memory 1, 2 (head wraps at once), 16 (valid bit 15); the
    linear objective (upd false on every accept); the constraint differences with ns = 33 (not dividing 64), 64 (column
    boundary on the lane 63 -> row 1 step), 1 (g1 = 0: the zero-norm branch, the second multiplier stays 0), 70 x 1
    and 10 x 2.
    Measured on the MI355X over the 19 cases: max |dc| 1.8e-15, max rel |df| 1.3e-16, max |dlam| 1.4e-13, every count
    equal to the host's."""
    from qoc_amd.optimize import minimize_ticks
    case = OC.BY_NAME[name]
    fg = case.make(DEV)
    c0 = case.c0(DEV)
    ref = minimize_ticks(fg, c0, **case.host_kw())
    assert ref.not_done == 0
    dev = run_device(fg, c0, ref.ticks + 2, **case.device_kw())  # two ticks more: finished seeds no longer change
    compare(dev, ref, fg(c0)[0])
    assert dev.rounds.tolist() == ref.rounds.tolist()
    if case.ns:
        dl = float((dev.lam - ref.lam).abs().max())
        dg = float((dev.g - ref.g).abs().max())
        print(f"max |dlam| = {dl:.3e}, |dg| = {dg:.3e}, lam {dev.lam.tolist()}, rho {dev.rho.tolist()}")
        assert dl <= 1e-6 and torch.equal(dev.rho, ref.rho)
        assert dev.rounds.tolist() == [3] * case.B and float(dev.lam.max()) > 0
        if case.ns == 1:  # the difference norm and its multiplier are exactly 0
            assert dev.g[:, 1].tolist() == [0.0] * case.B and dev.lam[:, 1].tolist() == [0.0] * case.B
    if name == "linear_box":
        assert float((dev.c.abs() - 0.5).abs().max()) == 0.0 and bool(dev.converged.all())


# ---- B. batch independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diagonal_n193_m10", "constrained_ns33_nu3"])
def test_a_seed_does_not_depend_on_its_batch_at_four_rows(built_lib, name):
    """The header of qoc_opt.hpp: a seed's iterates depend on nothing but its own data.  Seed 1 of the case alone
    (seed 0 of a workgroup's first wave) and as seed 2 of 3 (behind two other seeds): bitwise equal c, f, evals, with
    all four register rows (n = 193) and with the constraint differences (ns = 33, nu = 3)."""
    from qoc_amd.optimize import minimize_ticks
    case = OC.BY_NAME[name]
    pick = case.B - 1
    one = case.make(DEV, slice(pick, pick + 1))
    c1 = torch.zeros(1, case.n, dtype=torch.float64, device=DEV)
    ticks = minimize_ticks(one, c1, **case.host_kw()).ticks
    alone = run_device(one, c1, ticks, **case.device_kw())

    tt_fg = _gather(case, [0, 1, pick])  # the picked seed as seed 2 of 3, behind two other problems
    c3 = torch.zeros(3, case.n, dtype=torch.float64, device=DEV)
    full = run_device(tt_fg, c3, ticks + 3, **case.device_kw())
    assert bool(alone.done[0]) and bool(full.done[2])
    assert torch.equal(alone.c[0], full.c[2]) and torch.equal(alone.f[0], full.f[2])
    assert int(alone.evals[0]) == int(full.evals[2]) and int(alone.iters[0]) == int(full.iters[2])
    assert not torch.equal(full.c[0], full.c[2])  # the neighbours are other problems


def _gather(case, idx):
    """The case's objective with seeds idx[0], idx[1], ... as its batch (each seed's own elementwise arithmetic)."""
    parts = [case.make(DEV, slice(i, i + 1)) for i in idx]

    def fg(x):
        out = [p(x[k:k + 1]) for k, p in enumerate(parts)]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out], 0)
    return fg


# ---- C. the fused step through the engine ---------------------------------------------------------------------------
NU1 = dict(ZZ2, lower=-0.6, upper=0.6, g_upper=[1.2, 0.5])
ENGINE_CASES = {
    # the reference example's shape, 10 splines x 2 controls: nc = 20, second pass of the gradient loop (o0 += 16)
    "zz_Nt60_ns10": dict(system="zz", Nt=60, ns=10, B=3, kw=ZZ2),
    # Nt < 64: lanes 20..63 have no slice in the k = lane; k < Nt; k += 64 sums; nc = 18
    "zz_Nt20_ns9": dict(system="zz", Nt=20, ns=9, B=3, kw=ZZ2),
    # Nt nu = 300 > 256: second pass of the control-writing loop
    "zz_Nt150_ns10": dict(system="zz", Nt=150, ns=10, B=2, kw=ZZ2),
    # nu = 1, nc = 17: the last group of the gradient loop has one live slot of four
    "blocks_nu1_ns17": dict(system="blocks", Nt=40, ns=17, B=2, kw=NU1),
    # the same from c0 = 0: both norms are 0 at the first eval (zero Jacobian rows, not NaN)
    "blocks_nu1_ns17_zero_start": dict(system="blocks", Nt=40, ns=17, B=2, kw=NU1, zero=True),
}


def _engine_case(spec):
    from qoc_amd import GrapeEngine, systems
    B, Nt, ns = spec["B"], spec["Nt"], spec["ns"]
    if spec["system"] == "zz":
        prob = systems.zz_problem(Nt)
        rng = np.random.default_rng(1)  # the starts of test_gpu_optimize_device._zz_engine
        c0 = np.concatenate([0.01 * np.ones((B, ns)), np.zeros((B, ns))], 1) + 0.01 * rng.standard_normal((B, 2 * ns))
    else:
        import blkseg_util
        prob = blkseg_util.block_problem(2, 7, 1, 3, Nt=Nt, seed=21)[0]
        c0 = 0.2 * np.random.default_rng(21).standard_normal((B, ns))
        if spec.get("zero"):
            c0 = np.zeros((B, ns))
    Bs = systems.spline_matrix(10.0, Nt, ns)
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    return e, Bs, c0


def _c3(c, ns, nu):
    """(B, nc) in the optimiser's layout (s + ns j) -> eval_spline's (B, ns, nu)."""
    c = c.cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
    return c.reshape(c.shape[0], nu, ns).transpose(0, 2, 1)


def _unfused(e, ns, nu, c0d, ticks, kw):
    """eval_spline_device at the trials, then the generic tell kernel (the same opt_tell), on the engine's stream."""
    from qoc_amd.optimize import DeviceOptimizer
    B = c0d.shape[0]
    opt = DeviceOptimizer(B, ns * nu, ns=ns, nu=nu, device=0, stream=e.stream(), **kw)
    J = torch.empty(B, dtype=torch.float64, device=DEV)
    G = torch.empty(B, ns * nu, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    opt.start(c0d)
    for _ in range(ticks):
        e.eval_spline_device(opt.trial_ptr(), 3, J.data_ptr(), G.data_ptr())
        opt.tell(J.data_ptr(), G.data_ptr())
    res = opt.result()
    opt.close()
    return res


@pytest.fixture(scope="module", params=list(ENGINE_CASES))
def engine_run(built_lib, request):
    """One fused run, its host reference, the same run unfused, the closing eval's best seed and the eval again at the
    returned iterates, on one engine."""
    from qoc_amd.optimize import SplineGrape, minimize_on_device, minimize_ticks
    spec = ENGINE_CASES[request.param]
    e, Bs, c0 = _engine_case(spec)
    sg = SplineGrape(e, Bs)
    ns, nu, kw = sg.ns, sg.nu, spec["kw"]
    assert (ns, nu * ns) == (spec["ns"], c0.shape[1])
    c0d = torch.from_numpy(c0).to(DEV)
    ref = minimize_ticks(sg.fg, c0d, cons=sg.cons, **kw)
    dev = minimize_on_device(e, Bs, c0d, **kw)
    best = e.allgather_best()
    J_again = e.eval_spline(_c3(dev.c, ns, nu))[0]
    unfused = _unfused(e, ns, nu, c0d, dev.ticks, kw)
    e.close()
    return dict(name=request.param, spec=spec, ref=ref, dev=dev, best=best, J_again=J_again, unfused=unfused, nu=nu)


def test_fused_step_shapes_against_host_machine(engine_run):
    """k_opt_step_spline against minimize_ticks(SplineGrape.fg, cons=SplineGrape.cons): nc = 20 and 18 (second pass of
    for (o0 = wave; o0 < nc; o0 += 16)), Nt = 20 (lanes without a slice), Nt nu = 300 (second pass of the
    control-writing loop), nu = 1 with nc = 17 (one live slot in the last group of four), and the zero start.
    Measured on the MI355X over the five cases: max |dc| 4.2e-16, |df| 2.3e-16, |dlam| 1.2e-14; 21 to 32 ticks; in the
    first case lam reaches 0.33 and rho is raised to 100 on two seeds."""
    r = engine_run
    dev, ref, kw = r["dev"], r["ref"], r["spec"]["kw"]
    print(r["name"], "iters", dev.iters.tolist(), "rounds", dev.rounds.tolist(), "lam max", float(dev.lam.max()),
          "rho", dev.rho.tolist())
    _zz_compare(dev, ref)
    assert dev.ls_fails.tolist() == ref.ls_fails.tolist() and dev.converged.tolist() == ref.converged.tolist()
    assert dev.rounds.tolist() == [3] * r["spec"]["B"]
    assert int(dev.iters.min()) > 0  # from c0 = 0 too: the gradient at u = 0 is not zero
    assert float(dev.c.abs().max()) <= kw["upper"]
    if r["name"] == "zz_Nt60_ns10":  # a constraint becomes active and the penalty is raised
        assert float(dev.lam.max()) > 0 and float(dev.rho.max()) > 10.0


def test_fused_step_shapes_equal_the_unfused_run(engine_run):
    """The fused gradient (k_spline_grad's order inside k_opt_step_spline) and the fused control writing (k_spline_u's
    order) against eval_spline_device + the generic tell: bit for bit at every shape of ENGINE_CASES."""
    dev, unf = engine_run["dev"], engine_run["unfused"]
    assert dev.evals.tolist() == unf.evals.tolist() and dev.iters.tolist() == unf.iters.tolist()
    assert torch.equal(dev.c, unf.c) and torch.equal(dev.f, unf.f)
    assert torch.equal(dev.lam, unf.lam) and torch.equal(dev.rho, unf.rho) and torch.equal(dev.g, unf.g)


def test_closing_eval_and_best_seed_at_every_shape(engine_run):
    """res.f is the eval at the returned c (k_spline_u maps the same c the fused step mapped) and allgather_best() is
    (min f, argmin) of the closing eval."""
    f = engine_run["dev"].f.cpu().numpy()
    assert np.array_equal(f, engine_run["J_again"])
    Jb, sb = engine_run["best"]
    assert Jb == f.min() and sb == int(f.argmin())


# ---- D. the host loop of qoc_minimize_spline_dev -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_loop(built_lib):
    from qoc_amd.optimize import minimize_on_device
    spec = ENGINE_CASES["zz_Nt60_ns10"]
    e, Bs, c0 = _engine_case(spec)
    ns, nu, B = spec["ns"], 2, spec["B"]
    c0d = torch.from_numpy(c0).to(DEV)

    def run(c=c0d, **kw):
        res = minimize_on_device(e, Bs, c, **dict(ZZ2, **kw))
        return dict(res=res, best=e.allgather_best(), J_again=e.eval_spline(_c3(res.c, ns, nu))[0])
    out = dict(B=B, full=run())
    for p in (1, 3):
        out[f"poll{p}"] = run(poll_every=p)
    ev = out["full"]["res"].evals
    lo, hi = int(ev.min()), int(ev.max())
    cut = (lo + hi) // 2
    out["cut"] = cut
    out["cut_run"] = run(max_ticks=cut, poll_every=16)
    out["cut_poll"] = 3 if cut % 3 else 4  # max_ticks is not a multiple of poll_every: the last group is shorter
    out["cut_run_uneven"] = run(max_ticks=cut, poll_every=out["cut_poll"])
    out["cut7"] = run(max_ticks=7, poll_every=3)
    big = torch.from_numpy(30.0 * c0).to(DEV)  # entries beyond the bounds +-0.2
    out["c0_big"] = big
    out["zero"] = run(c=big, max_ticks=0)
    e.close()
    return out


def test_poll_every_does_not_change_the_run(host_loop):
    """poll_every = 1, 3, 16: the host sees the finished-seed count one tick late (opt_mirror_done), so with
    poll_every = 1 it queues one tick more than the slowest seed needs; finished seeds do not change, so c, f, lam are
    bitwise equal, the counts equal, and ticks_out is max(evals) in every run."""
    full = host_loop["full"]["res"]
    assert full.not_done == 0 and full.ticks == int(full.evals.max())
    assert len(set(full.evals.tolist())) > 1
    for p in (1, 3):
        r = host_loop[f"poll{p}"]["res"]
        assert torch.equal(r.c, full.c) and torch.equal(r.f, full.f) and torch.equal(r.lam, full.lam)
        assert torch.equal(r.rho, full.rho)
        for k in ("evals", "iters", "rounds", "ls_fails", "converged", "done"):
            assert getattr(r, k).tolist() == getattr(full, k).tolist(), (p, k)
        assert r.ticks == full.ticks and r.not_done == 0
        assert host_loop[f"poll{p}"]["best"] == host_loop["full"]["best"]


@pytest.mark.parametrize("which", ["cut_run", "cut_run_uneven", "cut7"])
def test_max_ticks_below_the_need_on_the_device(host_loop, which):
    """The device twin of test_optimize_ticks.py::test_max_ticks_below_the_need: a seed that finishes stops counting,
    the others stop at max_ticks; the group split min(poll_every, max_ticks - ticks) with max_ticks a multiple of
    poll_every or not (cut and poll 3 or 4; 7 and 3)."""
    full = host_loop["full"]["res"]
    cut = 7 if which == "cut7" else host_loop["cut"]
    if which != "cut7":
        assert int(full.evals.min()) < cut < int(full.evals.max())
    if which == "cut_run_uneven":
        assert cut % host_loop["cut_poll"] != 0
    r = host_loop[which]["res"]
    print(which, "cut", cut, "evals", r.evals.tolist(), "of", full.evals.tolist())
    assert r.evals.tolist() == [min(int(v), cut) for v in full.evals]
    assert r.not_done == int((full.evals > cut).sum()) > 0
    assert r.done.tolist() == (full.evals <= cut).tolist()
    assert r.ticks == cut
    assert float(r.c.abs().max()) <= 0.2
    f = r.f.cpu().numpy()
    assert np.array_equal(f, host_loop[which]["J_again"])
    Jb, sb = host_loop[which]["best"]
    assert Jb == f.min() and sb == int(f.argmin())
    # a seed that was done before the cut is where the full run left it
    for b in range(host_loop["B"]):
        if int(full.evals[b]) <= cut:
            assert torch.equal(r.c[b], full.c[b]) and torch.equal(r.f[b], full.f[b])


def test_max_ticks_zero_returns_the_clamped_start(host_loop):
    """max_ticks = 0: no tick runs; the result is clamp(c0) with evals = 0, nothing done, and f of the closing eval at
    those coefficients."""
    r = host_loop["zero"]["res"]
    c0 = host_loop["c0_big"]
    assert float(c0.abs().max()) > 0.2
    assert torch.equal(r.c, c0.clamp(-0.2, 0.2))
    assert r.evals.tolist() == [0] * host_loop["B"] and r.iters.tolist() == [0] * host_loop["B"]
    assert r.ticks == 0 and r.not_done == host_loop["B"] and not bool(r.done.any())
    f = r.f.cpu().numpy()
    assert np.isfinite(f).all() and (f > 0).all()
    assert np.array_equal(f, host_loop["zero"]["J_again"])
    Jb, sb = host_loop["zero"]["best"]
    assert Jb == f.min() and sb == int(f.argmin())
