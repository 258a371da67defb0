"""GPU: the device optimiser with the gate duration as every seed's last variable (include/qoc.h
qoc_opt_create_duration, qoc_minimize_spline_duration_dev; csrc/qoc_opt.hpp opt_tell<true>, k_opt_step_spline_dur)
against its host reference: qoc_amd.optimize.minimize_ticks with per-variable bounds and, for the spline norms,
a constraint closure whose τ column is zero.

The bars are those of tests/test_gpu_optimize_device.py, whose ``compare`` and ``_zz_compare`` are used as they are:
equal per-seed counts and ticks; c 1e-9 and f 1e-12 relative for the analytic problems; c 1e-8, f 1e-10, lam 1e-6 and
equal rho for zz.  The fused run against the same run as ask / tell, a seed alone against the seed in a batch, and the
result's f against a fresh eval are compared bit for bit.

Observed on an MI355X: the analytic cases with equal counts, max |Δc| 5.2e-14, relative |Δf| 4.5e-17, |Δλ| 4.0e-13; zz
free |Δc| 5.7e-16, |Δf| 1.1e-15; zz constrained |Δc| 3.9e-14, |Δf| 2.8e-14, |Δλ| 3.8e-13; J against the oracle 2.2e-15.
"""
import numpy as np
import pytest
import torch

import qoc_oracle as O
from blkseg_util import case
from test_gpu_optimize_device import _zz_compare, ball, compare, quadratic, rosen, run_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAU = (0.5, 2.0)  # the duration's bounds; every scalar bound of a c part below differs from both


def _dur_cons(ns, nu):
    from qoc_amd.optimize import duration_constraints_torch
    return lambda z: duration_constraints_torch(z, ns, nu)


def _vec_bounds(n, lower, upper, tau):
    lo = np.concatenate([np.full(n - 1, -np.inf if lower is None else lower), [tau[0]]])
    hi = np.concatenate([np.full(n - 1, np.inf if upper is None else upper), [tau[1]]])
    return lo, hi


def diagonal_dur(n, dev=DEV):
    """0.5 Σ_i d_i (z_i - t_bi)², three seeds.  The last variable's targets 0.2, 3.0 and 1.2 put its minimiser on
    tau_lower, on tau_upper and strictly inside [0.5, 2]; the c targets (1.5 N(0, 1)) put c variables on ±1."""
    torch.manual_seed(3)
    dg = torch.linspace(1, 25, n, dtype=torch.float64).to(dev)
    tt = 1.5 * torch.randn(3, n, dtype=torch.float64)
    tt[:, n - 1] = torch.tensor([0.2, 3.0, 1.2], dtype=torch.float64)
    tt = tt.to(dev)

    def fg(x):
        return 0.5 * (dg * (x - tt) ** 2).sum(1), dg * (x - tt)
    return fg


def _diag_start(n):
    z0 = np.zeros((3, n))
    z0[:, n - 1] = [1.0, 0.0, 5.0]  # the last two starts are clamped to tau_lower and tau_upper
    return z0


# name -> (objective, starts, minimize_ticks / DeviceOptimizer keywords, ns, nu, expected ends of the last variable)
CASES = {
    # n = 1: τ alone
    "diagonal_n1": (lambda dev=DEV: diagonal_dur(1, dev), _diag_start(1),
                    dict(lower=-1.0, upper=1.0, max_iter=30, gtol=1e-6), 0, 0, "lo hi in"),
    # n = 13 = 6 * 2 + 1 with both norm constraints
    "diagonal_n13_constrained": (lambda dev=DEV: diagonal_dur(13, dev), _diag_start(13),
                                 dict(lower=-1.0, upper=1.0, g_upper=[2.0, 2.5], max_iter=25, outer_iters=3, gtol=1e-6),
                                 6, 2, "lo hi in"),
    # n = 65 = 8 * 8 + 1: the duration is lane 0 of the second register row
    "diagonal_n65_constrained": (lambda dev=DEV: diagonal_dur(65, dev), _diag_start(65),
                                 dict(lower=-1.0, upper=1.0, g_upper=[5.0, 6.0], max_iter=25, outer_iters=2, gtol=1e-6),
                                 8, 8, "lo hi in"),
    # n = 256: the last lane of the last row
    "diagonal_n256": (lambda dev=DEV: diagonal_dur(256, dev), _diag_start(256),
                      dict(lower=-1.0, upper=1.0, max_iter=60, gtol=1e-6), 0, 0, "lo hi in"),
    # Rosenbrock with a <= 0.8: the minimiser is a = 0.8 on the scalar bound, the last variable a² = 0.64 inside
    "rosenbrock": (lambda dev=DEV: rosen, [[-1.2, 1.0], [0.0, 0.0], [2.0, 2.0], [0.5, 1.5]],
                   dict(lower=-1.5, upper=0.8, max_iter=300), 0, 0, "in in in in"),
    # +inf outside the unit ball: trials rejected for not being finite, failed line searches with max_ls = 2
    "ball_failed_line_searches": (lambda dev=DEV: ball, [[0.0, 0.9, 0.0], [-0.9, 0.0, 0.3], [0.1, 0.1, 0.95],
                                                         [0.0, 0.0, 0.0]],
                                  dict(max_iter=8, max_ls=2, gtol=1e-6), 0, 0, None),
}
BALL_TAU = (0.05, 0.5)


def _tau_of(name):
    return BALL_TAU if name.startswith("ball") else TAU


def reference_run(name, dev=DEV):
    """minimize_ticks alone, with what the case is meant to show asserted on it."""
    from qoc_amd.optimize import minimize_ticks
    mk, z0, kw, ns, nu, ends = CASES[name]
    fg = mk(dev)
    z0 = torch.tensor(np.asarray(z0), dtype=torch.float64, device=dev)
    n = z0.shape[1]
    tau = _tau_of(name)
    lo, hi = _vec_bounds(n, kw.get("lower"), kw.get("upper"), tau)
    hkw = {k: v for k, v in kw.items() if k not in ("lower", "upper")}
    ref = minimize_ticks(fg, z0, lower=lo, upper=hi, cons=_dur_cons(ns, nu) if ns else None, **hkw)
    assert ref.not_done == 0
    last = ref.c[:, n - 1].cpu().numpy()
    if ends is not None:
        for b, w in enumerate(ends.split()):
            if w == "lo":
                assert last[b] == tau[0]
            elif w == "hi":
                assert last[b] == tau[1]
            else:
                assert tau[0] < last[b] < tau[1]
    if n > 1 and "upper" in kw:  # a c variable on its scalar bound, which is neither of the duration's
        cpart = ref.c[:, :n - 1].cpu().numpy()
        assert (cpart <= kw["upper"]).all() and (cpart >= kw["lower"]).all()
        assert int((cpart == kw["upper"]).sum() + (cpart == kw["lower"]).sum()) > 0
        assert kw["upper"] not in tau and kw["lower"] not in tau
    if ns:
        assert float(ref.lam.max()) > 0  # a norm constraint is active
    if name.startswith("ball"):
        assert int(ref.ls_fails.max()) >= 1 and int(ref.iters.min()) >= 1
    return fg, z0, ref, kw, ns, nu, tau


@pytest.mark.parametrize("name", list(CASES))
def test_ask_tell_matches_host_state_machine(built_lib, name):
    fg, z0, ref, kw, ns, nu, tau = reference_run(name)
    dev = run_device(fg, z0, ref.ticks + 2, ns=ns, nu=nu, tau_bounds=tau, **kw)  # two ticks more: nothing changes
    compare(dev, ref, fg(z0)[0])
    n = z0.shape[1]
    # on a bound means the bound's own bits
    assert torch.equal(dev.c[:, n - 1] == tau[0], ref.c[:, n - 1] == tau[0])
    assert torch.equal(dev.c[:, n - 1] == tau[1], ref.c[:, n - 1] == tau[1])
    if ns:
        d = float((dev.lam - ref.lam).abs().max())
        print(f"max |dlam| = {d:.3e}, rounds {dev.rounds.tolist()}")
        assert dev.rounds.tolist() == ref.rounds.tolist() and torch.equal(dev.rho, ref.rho) and d <= 1e-6


def test_a_seed_does_not_depend_on_its_batch(built_lib):
    from qoc_amd.optimize import minimize_ticks
    kw = dict(lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6)
    tau = (0.05, 0.3)
    c0 = torch.zeros(5, 5, dtype=torch.float64, device=DEV)
    lo, hi = _vec_bounds(5, -0.5, 0.5, tau)
    ticks = minimize_ticks(quadratic(slice(0, 5)), c0, lower=lo, upper=hi, max_iter=200, gtol=1e-6).ticks
    full = run_device(quadratic(slice(0, 5)), c0, ticks, tau_bounds=tau, **kw)
    alone = run_device(quadratic(slice(2, 3)), c0[2:3].clone(), ticks, tau_bounds=tau, **kw)
    assert torch.equal(alone.c[0], full.c[2]) and torch.equal(alone.f[0], full.f[2])
    assert int(alone.evals[0]) == int(full.evals[2]) and bool(alone.done[0])
    assert float(full.c[:, 4].min()) >= tau[0] and float(full.c[:, 4].max()) <= tau[1]


# ---- zz through the engine: Nt = 60, ns = 6, nu = 2 (the shapes of test_gpu_duration.py's callers) --------------------
B, NS, NU = 5, 6, 2
NC = NS * NU
KAPPA = 0.05
TAU0 = np.array([0.8, 1.0, 1.25, 1.6, 2.4])  # the last start lies above tau_upper: the start clamp
ZKW = dict(max_iter=5)
ZKW_CONS = dict(g_upper=[0.55, 0.35], max_iter=5, outer_iters=3, rho0=10.0)


def _zz_engine(nB=B):
    from qoc_amd import GrapeEngine, systems
    prob = case("zz")[0]
    Bs = systems.spline_matrix(6.0, prob.Nt, NS)
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=nB)
    e.set_cost_trace(prob.x_target, prob.n)
    e.set_chain("taylor")
    return prob, Bs, e


def _zz_start():
    c0 = np.random.default_rng(97).uniform(-0.3, 0.3, size=(B, NS, NU))
    flat = c0.transpose(0, 2, 1).reshape(B, NC)
    return np.concatenate([flat, TAU0[:, None]], 1)


def _unfused(e, Bs, z0d, ticks, kw):
    """The run as ask / tell, everything queued on the engine's stream: eval_spline_device on the contiguous c part, τ
    copied into the engine's buffer, f and grad formed in torch."""
    from qoc_amd.optimize import DeviceOptimizer, _DevView
    okw = dict(kw)
    if "g_upper" not in okw:
        okw.update(g_upper=(np.inf, np.inf), outer_iters=1)
    opt = DeviceOptimizer(B, NC + 1, -0.4, 0.4, ns=NS, nu=NU, device=0, stream=e.stream(), tau_bounds=TAU,
                          time_weight=KAPPA, **okw)
    torch.cuda.synchronize()
    e.synchronize()
    with torch.cuda.stream(torch.cuda.ExternalStream(e.stream())):
        J = torch.empty(B, dtype=torch.float64, device=DEV)
        G = torch.empty(B, NC, dtype=torch.float64, device=DEV)
        tau = torch.as_tensor(_DevView(e.time_scale_device(), (B,), "<f8"), device=DEV)
        dtau = torch.as_tensor(_DevView(e.time_scale_grad_device(), (B,), "<f8"), device=DEV)
        opt.start(z0d)
        xt = opt.trial
        for _ in range(ticks):
            c = xt[:, :NC].contiguous()
            tau.copy_(xt[:, NC])
            e.eval_spline_device(c.data_ptr(), 3, J.data_ptr(), G.data_ptr())
            opt.tell(J + KAPPA * xt[:, NC], torch.cat([G, (dtau + KAPPA)[:, None]], 1))
        res = opt.result()
    torch.cuda.synchronize()
    opt.close()
    return res


@pytest.fixture(scope="module")
def zz_runs(built_lib):
    """One engine: the host machine, the fused run and the same run as ask / tell, unconstrained and constrained; what
    the closing eval left; a run with max_ticks = 0."""
    from qoc_amd.optimize import SplineGrapeDuration, _DevView, minimize_duration_on_device, minimize_ticks
    prob, Bs, e = _zz_engine()
    z0 = _zz_start()
    z0d = torch.from_numpy(z0).to(DEV)
    lo, hi = _vec_bounds(NC + 1, -0.4, 0.4, TAU)
    obj = SplineGrapeDuration(e, Bs, order=3, time_weight=KAPPA)
    out = dict(prob=prob, Bs=Bs, z0=z0)
    for key, kw in (("free", ZKW), ("cons", ZKW_CONS)):
        # "free": the norms unbounded in one round, which is what g_upper = None means on the device
        hkw = kw if "g_upper" in kw else dict(kw, g_upper=[np.inf, np.inf], outer_iters=1)
        ref = minimize_ticks(obj.fg, z0d, lower=lo, upper=hi, cons=obj.cons, **hkw)
        ref_none = None if "g_upper" in kw else minimize_ticks(obj.fg, z0d, lower=lo, upper=hi, **kw)
        dev = minimize_duration_on_device(e, Bs, z0d, -0.4, 0.4, TAU, KAPPA, **kw)
        # what the closing eval left, before anything else runs on the engine
        tau_buf = torch.as_tensor(_DevView(e.time_scale_device(), (B,), "<f8"), device=DEV).cpu().numpy().copy()
        best = e.allgather_best()
        zf = dev.c.cpu().numpy()
        J_again = e.eval_spline(zf[:, :NC].reshape(B, NU, NS).transpose(0, 2, 1))[0]  # τ is still the run's
        unf = _unfused(e, Bs, z0d, dev.ticks, kw)
        out[key] = dict(ref=ref, ref_none=ref_none, dev=dev, tau_buf=tau_buf, best=best, J_again=J_again, unf=unf)
    zero = minimize_duration_on_device(e, Bs, z0d, -0.4, 0.4, TAU, KAPPA, max_ticks=0, **ZKW)
    tau_zero = torch.as_tensor(_DevView(e.time_scale_device(), (B,), "<f8"), device=DEV).cpu().numpy().copy()
    zc = zero.c.cpu().numpy()
    J_zero = e.eval_spline(zc[:, :NC].reshape(B, NU, NS).transpose(0, 2, 1))[0]
    out["zero"] = dict(res=zero, tau_buf=tau_zero, J=J_zero)
    e.close()
    return out


@pytest.mark.parametrize("key", ["free", "cons"])
def test_zz_fused_run_against_host_machine(zz_runs, key):
    dev, ref = zz_runs[key]["dev"], zz_runs[key]["ref"]
    _zz_compare(dev, ref)
    if key == "free":
        # unbounded norms are no constraint: the host machine without a constraint closure takes the same steps
        none = zz_runs[key]["ref_none"]
        assert torch.equal(none.c, ref.c) and torch.equal(none.f, ref.f) and none.evals.tolist() == ref.evals.tolist()
        assert float(dev.lam.abs().max()) == 0.0
    tau = dev.c[:, NC].cpu().numpy()
    assert (tau >= TAU[0]).all() and (tau <= TAU[1]).all() and float(dev.c[:, :NC].abs().max()) <= 0.4
    assert (tau[:4] != TAU0[:4]).all()  # the durations that started inside moved: τ is a variable
    if key == "cons":
        assert dev.rounds.tolist() == [3] * B
        assert float(dev.lam.max()) > 0 and float(dev.rho.max()) > 10.0  # a constraint is active, the penalty was raised


def test_start_clamp_is_seen(zz_runs):
    """Seed 4 starts at τ = 2.4 > tau_upper; with no tick run the iterate is the clamped start."""
    z = zz_runs["zero"]["res"].c.cpu().numpy()
    want = zz_runs["z0"].copy()
    want[:, NC] = np.clip(want[:, NC], *TAU)
    want[:, :NC] = np.clip(want[:, :NC], -0.4, 0.4)
    assert np.array_equal(z, want) and z[4, NC] == TAU[1] and zz_runs["z0"][4, NC] > TAU[1]


@pytest.mark.parametrize("key", ["free", "cons"])
def test_fused_step_is_the_unfused_run(zz_runs, key):
    dev, unf = zz_runs[key]["dev"], zz_runs[key]["unf"]
    assert torch.equal(dev.c, unf.c) and torch.equal(dev.f, unf.f)
    assert torch.equal(dev.lam, unf.lam) and dev.evals.tolist() == unf.evals.tolist()
    assert int(dev.iters.min()) >= 1


@pytest.mark.parametrize("key", ["free", "cons"])
def test_closing_eval(zz_runs, key):
    r = zz_runs[key]
    dev = r["dev"]
    z = dev.c.cpu().numpy()
    tau = z[:, NC]
    # f was evaluated on the fused step's u and τ; eval_spline maps the same c with k_spline_u under the τ the run left
    assert np.array_equal(r["tau_buf"], tau)
    assert np.array_equal(dev.f.cpu().numpy(), r["J_again"] + KAPPA * tau)
    Jb, sb = r["best"]  # the closing eval's own: the minimum of J, not of f
    assert Jb == r["J_again"].min() and sb == int(r["J_again"].argmin())


def test_no_tick_gives_the_closing_eval_at_the_clamped_start(zz_runs):
    r = zz_runs["zero"]
    res = r["res"]
    tau = res.c[:, NC].cpu().numpy()
    assert res.ticks == 0 and res.evals.tolist() == [0] * B and res.not_done == B
    assert np.array_equal(r["tau_buf"], tau)
    assert np.array_equal(res.f.cpu().numpy(), r["J"] + KAPPA * tau)


def test_returned_cost_against_the_cpu_oracle(zz_runs):
    """J of the fresh eval at one returned (c, τ) (bitwise the result's f - κτ, test_closing_eval) against the oracle on
    the τ-scaled generators, at test_gpu_duration.py's bar."""
    prob, Bs = zz_runs["prob"], zz_runs["Bs"]
    z = zz_runs["free"]["dev"].c.cpu().numpy()
    b = 2
    uf = np.einsum("tn,nj->jt", Bs, z[b, :NC].reshape(NU, NS).T)
    t = z[b, NC]
    Jr = O.grape_eval(t * prob.A0, [t * a for a in prob.A], uf, prob.x0, prob.x_target, prob.n)[0]
    J = zz_runs["free"]["J_again"][b]
    print("dJ", J - Jr)
    assert abs(J - Jr) <= 1e-12 * max(1.0, abs(Jr))


def _raises(code, f, *a, **k):
    from qoc_amd import QOCError
    with pytest.raises(QOCError) as ei:
        f(*a, **k)
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


def test_refusals_change_nothing(built_lib, monkeypatch):
    from qoc_amd import _lib
    from qoc_amd.optimize import DeviceOptimizer, _DevView, minimize_duration_on_device
    un, st, ar = _lib.QOC_ERR_UNSUPPORTED, _lib.QOC_ERR_STATE, _lib.QOC_ERR_ARG
    prob, Bs, e = _zz_engine()
    z0d = torch.from_numpy(_zz_start()).to(DEV)
    run = lambda: minimize_duration_on_device(e, Bs, z0d, -0.4, 0.4, TAU, KAPPA, **ZKW)  # noqa: E731
    first = run()

    okw = dict(ns=NS, nu=NU, g_upper=(np.inf, np.inf), outer_iters=1, device=0, stream=e.stream(), **ZKW)
    dur = DeviceOptimizer(B, NC + 1, -0.4, 0.4, tau_bounds=TAU, time_weight=KAPPA, **okw)
    dur3 = DeviceOptimizer(3, NC + 1, -0.4, 0.4, tau_bounds=TAU, time_weight=KAPPA, **okw)
    plain = DeviceOptimizer(B, NC, -0.4, 0.4, **okw)
    zs = torch.full((B, NC + 1), 7.25, dtype=torch.float64, device=DEV)
    cs = torch.full((B, NC), 7.25, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()

    def sentinel_tau():
        t = torch.as_tensor(_DevView(e.time_scale_device(), (B,), "<f8"), device=DEV)
        t.fill_(1.375)
        torch.cuda.synchronize()
        return t

    def untouched(t):
        e.synchronize()
        torch.cuda.synchronize()
        assert bool((zs == 7.25).all()) and bool((cs == 7.25).all())
        if t is not None:
            assert bool((t == 1.375).all())

    # no time scale
    e.set_time_scale(None)
    _raises(st, e.minimize_spline_duration_device, dur, zs.data_ptr(), 10)
    untouched(None)
    assert e.time_scale_device() == 0
    e.set_time_scale(np.ones(B))
    t = sentinel_tau()
    # the object kinds crossed, both ways; another B
    _raises(ar, e.minimize_spline_duration_device, plain, zs.data_ptr(), 10)
    _raises(ar, e.minimize_spline_device, dur, cs.data_ptr(), 10)
    _raises(ar, e.minimize_spline_duration_device, dur3, zs.data_ptr(), 10)
    untouched(t)
    # an external cost; a co-state source; QOC_BLKSEG=0
    e.set_cost_external()
    _raises(st, e.minimize_spline_duration_device, dur, zs.data_ptr(), 10)
    e.set_cost_trace(prob.x_target, prob.n)
    untouched(t)
    e.set_costate_source(np.zeros((B, prob.Nt + 1, prob.N, prob.m), complex))
    _raises(un, e.minimize_spline_duration_device, dur, zs.data_ptr(), 10)
    e.set_costate_source(None)
    untouched(t)
    monkeypatch.setenv("QOC_BLKSEG", "0")
    _raises(un, e.minimize_spline_duration_device, dur, zs.data_ptr(), 10)
    monkeypatch.delenv("QOC_BLKSEG")
    untouched(t)
    for o in (dur, dur3, plain):
        o.close()

    again = run()
    assert torch.equal(again.c, first.c) and torch.equal(again.f, first.f)
    assert again.evals.tolist() == first.evals.tolist() and again.ticks == first.ticks
    e.close()
