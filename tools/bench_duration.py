"""Gate-duration evals (diagnostic, plain timing), in evals per second:
  flag    what the TS kernels cost: eval_device with set_time_scale(1 for every seed) against the plain eval of the
          same build, on two contexts whose timed repeats alternate (plain, scaled, plain, scaled, ...);
          cavity (N = 40, Nt = 1000, B = 256) and zz (N = 9, Nt = 500, B = 512), with and without the state penalty,
          order 3 and exact
  sweep   what a gate-time sweep gains: 16 durations x 16 seeds in one context (B = 256, set_time_scale) against the
          caller's form without it, 16 contexts of B = 16 with τ-scaled generators evaluated back to back (each waits
          for the one before it through an event: one stream's order), cavity and zz, order 3
  optimise  time-optimal control end to end on zz (N = 9, Nt = 500, B = 512, 10 splines, order 3 and exact), z = [c, τ],
          f = J + 0.05 τ, |c| <= 0.4, 0.5 <= τ <= 2, the same starts and the same number of ticks (--ticks, 600; gtol = 0, so no seed stops early) in:
          (a) the host-driven drivers over SplineGrapeDuration.fg with a device z: minimize_ticks stopped after that many
              ticks, and minimize_batched with as many iterations as give about that many batched evals
          (b) minimize_on_device at fixed τ (the starts' own), stopped after that many ticks
          (c) minimize_duration_on_device stopped after that many ticks
          one warm-up of every leg, then 3 rounds in which the legs take turns; ticks/s of every repeat, and for (a) and
          (c) the accepted iterations per seed and the best f
Warm-up of 20 steps, then K = 200 timed steps between two synchronisations, 3 repeats, every repeat printed, one
process at a time.
--parent DIR times the package of another checkout (built there) with this tool: a library from before the time scale
has the plain and the contexts legs only.
Usage: python tools/bench_duration.py [flag|sweep|optimise ...] [--steps K] [--ticks T] [--parent DIR]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--parent" in sys.argv:
    _i = sys.argv.index("--parent")
    ROOT = os.path.abspath(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from qoc_amd import GrapeEngine, systems  # noqa: E402

args = sys.argv[1:]
K = 200
if "--steps" in args:
    _i = args.index("--steps")
    K = max(1, int(args[_i + 1]))
    del args[_i:_i + 2]
TICKS = 600
if "--ticks" in args:
    _i = args.index("--ticks")
    TICKS = max(1, int(args[_i + 1]))
    del args[_i:_i + 2]
WARM, REPEATS = 20, 3
parts = args or ["flag", "sweep"]
HAS_TS = hasattr(GrapeEngine, "set_time_scale")
MU = 0.37


def problem(cfg):
    mk_prob, mk_u, B = systems.CONFIGS["zz_batch" if cfg == "zz" else cfg]
    prob = mk_prob()
    if cfg == "zz":
        pen = (list(systems.QuantumBasis([3, 3])(["20", "21", "22"])), [0, 1, 2, 3], MU)
    else:  # the top two cavity levels of both qubit states
        h = prob.N // 2
        pen = ([h - 2, h - 1, 2 * h - 2, 2 * h - 1], [0, 1], MU)
    return prob, mk_u, B, pen


def make(prob, B, pen=None, tau=None, A0=None, A=None):
    e = GrapeEngine(prob.A0 if A0 is None else A0, prob.A if A is None else A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    if pen is not None:
        e.set_state_penalty(*pen)
    if tau is not None:
        e.set_time_scale(tau)
    return e


def bufs(prob, u):
    B = u.shape[0]
    return (torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda(),
            torch.empty(B, dtype=torch.float64, device="cuda"),
            torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device="cuda"))


def run(step, sync, units):
    sync()
    t = time.perf_counter()
    for _ in range(K):
        step()
    sync()
    return units * K / (time.perf_counter() - t)


def alternate(legs, units):
    """legs: {name: (step, sync)}; warm-up of each, then REPEATS rounds in which the legs take turns."""
    for step, sync in legs.values():
        for _ in range(WARM):
            step()
        sync()
    rates = {k: [] for k in legs}
    for _ in range(REPEATS):
        for k, (step, sync) in legs.items():
            rates[k].append(run(step, sync, units))
    return rates


def show(tag, rates):
    for k, r in rates.items():
        print(f"{tag} {k:9s} " + " ".join(f"{x / 1e6:.6f}" for x in r) + " M evals/s", flush=True)


def part_flag():
    for cfg in ("cavity", "zz"):
        prob, mk_u, B, pen = problem(cfg)
        u = mk_u(B, 0)
        for p in (None, pen):
            for order in (3, "exact"):
                legs, keep = {}, []
                for name, tau in (("plain", None), ("scaled", np.ones(B))):
                    if tau is not None and not HAS_TS:
                        continue
                    e = make(prob, B, p, tau)
                    ud, Jd, gd = bufs(prob, u)
                    keep.append((e, ud, Jd, gd))
                    legs[name] = ((lambda e=e, ud=ud, Jd=Jd, gd=gd: e.eval_device(ud.data_ptr(), order, Jd.data_ptr(),
                                                                                  gd.data_ptr())), e.synchronize)
                rates = alternate(legs, B)
                tag = f"flag {cfg} B={B} {'penalty' if p else 'no penalty'} order {order}"
                show(tag, rates)
                if "scaled" in rates:
                    print(f"{tag}: scaled / plain (medians) = {np.median(rates['scaled']) / np.median(rates['plain']):.3f}"
                          f"  J[0] plain {keep[0][2][0].item():.15g} scaled {keep[1][2][0].item():.15g}", flush=True)
                for e, *_ in keep:
                    e.close()


def part_sweep():
    nd, ns = 16, 16
    taus = np.linspace(0.5, 2.0, nd)
    for cfg in ("cavity", "zz"):
        prob, mk_u, _, _ = problem(cfg)
        u = mk_u(nd * ns, 0)  # seed b = 16 d + s runs duration d
        legs, keep = {}, []
        if HAS_TS:
            e = make(prob, nd * ns, None, np.repeat(taus, ns))
            ud, Jd, gd = bufs(prob, u)
            keep.append(e)
            legs["one batch"] = ((lambda: e.eval_device(ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())), e.synchronize)
        engs = [make(prob, ns, None, None, t * prob.A0, [t * a for a in prob.A]) for t in taus]
        streams = [torch.cuda.ExternalStream(x.stream()) for x in engs]
        bb = [bufs(prob, u[d * ns:(d + 1) * ns]) for d in range(nd)]
        last = [None]

        def step_ctx():
            for d in range(nd):
                if last[0] is not None:
                    streams[d].wait_event(last[0])
                engs[d].eval_device(bb[d][0].data_ptr(), 3, bb[d][1].data_ptr(), bb[d][2].data_ptr())
                last[0] = streams[d].record_event()

        def sync_ctx():
            for x in engs:
                x.synchronize()
        legs["contexts"] = (step_ctx, sync_ctx)
        rates = alternate(legs, nd * ns)
        tag = f"sweep {cfg} 16 durations x 16 seeds order 3"
        show(tag, rates)
        if HAS_TS:
            print(f"{tag}: one batch / contexts (medians) = "
                  f"{np.median(rates['one batch']) / np.median(rates['contexts']):.3f}"
                  f"  J[0] {Jd[0].item():.15g} contexts {bb[0][1][0].item():.15g}", flush=True)
        for x in keep + engs:
            x.close()


def part_optimise():
    from qoc_amd import optimize as opt
    has_dur = hasattr(opt, "minimize_duration_on_device")
    prob, _, B, _ = problem("zz")
    ns, nu, kappa = 10, prob.nu, 0.05
    nc = ns * nu
    Bs = systems.spline_matrix(20.0, prob.Nt, ns)  # zz_batch's gate time
    rng = np.random.default_rng(4)
    z0 = np.concatenate([rng.uniform(-0.3, 0.3, size=(B, nc)), rng.uniform(0.8, 1.6, size=(B, 1))], 1)
    z0d = torch.from_numpy(z0).cuda()
    c0d = z0d[:, :nc].contiguous()
    lo = np.concatenate([np.full(nc, -0.4), [0.5]])
    hi = np.concatenate([np.full(nc, 0.4), [2.0]])
    big = 10 ** 6  # iterations per round: no seed ends before the ticks run out
    for order in (3, "exact"):
        e = make(prob, B)
        e.set_time_scale(z0[:, nc])
        obj = opt.SplineGrapeDuration(e, Bs, order=order, time_weight=kappa)

        def host_ticks():
            r = opt.minimize_ticks(obj.fg, z0d, lower=lo, upper=hi, max_iter=big, gtol=0.0, max_ticks=TICKS)
            return r.ticks, r.iters.cpu().numpy(), float(r.f.min())

        def host_lockstep():  # a line search takes 1-2 batched evals here: TICKS / 2 iterations, the evals counted
            r = opt.minimize_batched(obj.fg, z0d, lower=lo, upper=hi, max_iter=max(1, TICKS // 2), gtol=0.0)
            return r.n_evals, np.full(B, len(r.history)), float(r.f.min())

        def fixed_tau():
            e.set_time_scale(z0[:, nc])
            r = opt.minimize_on_device(e, Bs, c0d, lower=-0.4, upper=0.4, max_iter=big, gtol=0.0, order=order, max_ticks=TICKS)
            return r.ticks, r.iters.cpu().numpy(), float(r.f.min())

        def duration():
            r = opt.minimize_duration_on_device(e, Bs, z0d, -0.4, 0.4, (0.5, 2.0), kappa, max_iter=big, gtol=0.0, order=order,
                                                max_ticks=TICKS)
            return r.ticks, r.iters.cpu().numpy(), float(r.f.min())

        legs = {"(a) host ticks": host_ticks, "(a) host lockstep": host_lockstep, "(b) device fixed tau": fixed_tau}
        if has_dur:
            legs["(c) device duration"] = duration
        rates, last = {k: [] for k in legs}, {}
        for rnd in range(-1, REPEATS):  # -1: warm-up
            for k, fn in legs.items():
                e.synchronize()
                torch.cuda.synchronize()
                t = time.perf_counter()
                last[k] = fn()
                e.synchronize()
                torch.cuda.synchronize()
                if rnd >= 0:
                    rates[k].append(last[k][0] / (time.perf_counter() - t))
        tag = f"optimise zz B={B} ns={ns} order {order} ticks {TICKS}"
        for k, r in rates.items():
            n, it, best = last[k]
            print(f"{tag} {k:21s} " + " ".join(f"{x:9.1f}" for x in r) + f" ticks/s  (batched evals {n})"
                  + ("" if k.startswith("(b)") else f"  accepted iterations per seed min {it.min()} median "
                     f"{np.median(it):.0f} max {it.max()}  best f {best:.9e}"), flush=True)
        med = {k: np.median(r) for k, r in rates.items()}
        print(f"{tag}: (b) / (a) host ticks = {med['(b) device fixed tau'] / med['(a) host ticks']:.1f}, (b) / (a) host "
              f"lockstep = {med['(b) device fixed tau'] / med['(a) host lockstep']:.1f}"
              + (f"; (c) / (a) host ticks = {med['(c) device duration'] / med['(a) host ticks']:.1f}, (c) / (a) host "
                 f"lockstep = {med['(c) device duration'] / med['(a) host lockstep']:.1f}, (c) / (b) = "
                 f"{med['(c) device duration'] / med['(b) device fixed tau']:.3f}" if has_dur else ""), flush=True)
        e.close()


torch.cuda.set_device(0)
for p in parts:
    {"flag": part_flag, "sweep": part_sweep, "optimise": part_optimise}[p]()
