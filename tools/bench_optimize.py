"""End-to-end multi-start optimisation, timed (diagnostic; bench.py stays the flagship measurement).

Settings of the reference driver (examples/zz_coupling_ipopt_exp.jl:56-80) on zz: Nt = 100, 10 splines,
|c| <= 2 pi 0.06, g_U = [2, 1], 150 L-BFGS iterations per round, B = 512 perturbed starts; and a cavity leg
(N = 40, Nt = 1000, 20 splines, |c| <= 0.05, B = 256); and a tunable-bus leg (N = 27, Nt = 2000, one flux control on
20 splines, 0.3 <= c <= 1.0 as tunable_bus_controls draws it, no norm constraints, B = 512).  In one process, alternating, REPEATS times each after a warm-up:
  (a) lockstep  minimize_batched on SplineGrape: batched torch on the host's schedule
  (b) device    minimize_on_device: per-seed state machines, one eval + one fused step kernel per tick
  (c) bare      as many eval_spline_device calls as (b) used ticks, one synchronisation at the end
Wall time is taken between device synchronisations.  Reported per leg: wall seconds of every repeat, batched evals or
ticks, seed-evals/s, iterations/s, best f; and (b)/(c), the cost of a tick over a bare eval, and the share of (b)'s
seed-ticks spent on seeds that were already done.  Writes profiles/bench_optimize_<tag>.json.
--order 3|exact: the gradient every leg runs on (dUkdp_order; "exact" is the derivative of the computed f, and on these
two systems stays on the segmented eval, on the tunable bus on the interpolating block propagators); the device leg also reports its failed line searches and their share of its
seed-ticks (each failed search spends max_ls = 12 trials).
Usage: python tools/bench_optimize.py [zz|cavity|tunable_bus ...] [--tag TAG] [--repeats R] [--B B] [--max-iter K] [--outer R]
       [--order 3|exact]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from qoc_amd import GrapeEngine, systems  # noqa: E402
from qoc_amd.optimize import SplineGrape, minimize_batched, minimize_on_device  # noqa: E402


def opt(args, name, default, cast=int):
    if name in args:
        i = args.index(name)
        v = cast(args[i + 1])
        del args[i:i + 2]
        return v
    return default


args = sys.argv[1:]
TAG = opt(args, "--tag", "run", str)
REPEATS = opt(args, "--repeats", 3)
B_OVERRIDE = opt(args, "--B", 0)
MAX_ITER = opt(args, "--max-iter", 150)
OUTER = opt(args, "--outer", 2)
ORDER = opt(args, "--order", "3", str)
ORDER = "exact" if ORDER == "exact" else int(ORDER)
MAX_LS = 12  # minimize_on_device's default
cfgs = args or ["zz", "cavity"]


def setup(cfg):
    rng = np.random.default_rng(2)
    if cfg == "zz":
        prob, ns, B = systems.zz_problem(100), 10, B_OVERRIDE or 512
        Bs = systems.spline_matrix(10.0, prob.Nt, ns)
        bound = 2 * np.pi * 0.060
        c0 = np.concatenate([0.01 * np.ones((B, ns)), np.zeros((B, ns))], 1) + 0.02 * rng.standard_normal((B, 2 * ns))
    elif cfg == "tunable_bus":
        prob, ns, B = systems.CONFIGS["tunable_bus"][0](), 20, B_OVERRIDE or 512
        Bs = systems.spline_matrix(350.0, prob.Nt, ns)
        c0 = rng.uniform(0.4, 0.9, size=(B, ns))
        return prob, Bs, c0, B, dict(lower=0.3, upper=1.0, max_iter=MAX_ITER, outer_iters=1)
    else:
        prob, ns, B = systems.CONFIGS["cavity"][0](), 20, B_OVERRIDE or 256
        Bs = systems.spline_matrix(float(prob.Nt), prob.Nt, ns)
        bound = 0.05
        c0 = 0.01 * rng.standard_normal((B, 2 * ns))
    kw = dict(lower=-bound, upper=bound, g_upper=[2.0, 1.0], max_iter=MAX_ITER, outer_iters=OUTER)
    return prob, Bs, c0, B, kw


def sync(eng):
    eng.synchronize()
    torch.cuda.synchronize()


def run(cfg):
    prob, Bs, c0, B, kw = setup(cfg)
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    eng.set_cost_trace(prob.x_target, prob.n)
    sg = SplineGrape(eng, Bs, order=ORDER)
    c0d = torch.from_numpy(c0).cuda()
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    Gd = torch.empty(B, c0.shape[1], dtype=torch.float64, device="cuda")
    state = {"ticks": 0}

    def lockstep():
        r = minimize_batched(sg.fg, c0d, cons=sg.cons if "g_upper" in kw else None, **kw)
        return dict(batched_evals=r.n_evals, seed_evals=B * r.n_evals, iterations=B * len(r.history),
                    best_f=float(r.f.min()), converged=int(r.converged.sum()))

    def device():
        r = minimize_on_device(eng, Bs, c0d, order=ORDER, **kw)
        state["ticks"] = r.ticks
        ev = r.evals.cpu().numpy()
        return dict(batched_evals=r.ticks, seed_evals=int(ev.sum()), iterations=int(r.iters.sum()),
                    best_f=float(r.f.min()), converged=int(r.converged.sum()), not_done=r.not_done,
                    ls_fails=int(r.ls_fails.sum()),
                    ls_fail_tick_share=float(MAX_LS * int(r.ls_fails.sum()) / max(int(ev.sum()), 1)),
                    evals_min=int(ev.min()), evals_median=float(np.median(ev)), evals_max=int(ev.max()),
                    done_seed_tick_share=float(1.0 - ev.mean() / max(r.ticks, 1)), best=eng.allgather_best())

    def bare():
        for _ in range(state["ticks"]):
            eng.eval_spline_device(c0d.data_ptr(), ORDER, Jd.data_ptr(), Gd.data_ptr())
        return dict(batched_evals=state["ticks"], seed_evals=B * state["ticks"])

    legs = (("lockstep", lockstep), ("device", device), ("bare", bare))
    out = {name: {"wall_s": []} for name, _ in legs}
    for rep in range(-1, REPEATS):  # -1: warm-up
        for name, fn in legs:
            sync(eng)
            t = time.perf_counter()
            res = fn()
            sync(eng)
            dt = time.perf_counter() - t
            if rep < 0:
                continue
            out[name]["wall_s"].append(dt)
            out[name].update(res)
            print(f"{cfg} {name:8s} rep {rep}: {dt * 1e3:9.2f} ms  batched evals {res['batched_evals']:5d}  "
                  f"{res['seed_evals'] / dt / 1e6:7.3f} M seed-evals/s"
                  + (f"  {res['iterations'] / dt / 1e3:8.1f} k iterations/s  best f {res['best_f']:.6e}"
                     if "iterations" in res else "")
                  + (f"  failed line searches {res['ls_fails']} ({res['ls_fail_tick_share']:.1%} of the seed-ticks)"
                     if "ls_fails" in res else ""), flush=True)
    info = eng.info()
    eng.close()
    a, b, c = (out[k]["wall_s"] for k in ("lockstep", "device", "bare"))
    out["device_over_bare"] = [x / y for x, y in zip(b, c)]
    out["lockstep_best_over_device_worst"] = min(a) / max(b)
    out["every_device_repeat_beats_best_lockstep"] = bool(max(b) < min(a))
    out["settings"] = dict(cfg=cfg, B=B, N=prob.N, Nt=prob.Nt, ns=Bs.shape[1], max_iter=MAX_ITER, outer_iters=kw["outer_iters"],
                           order=ORDER, backward=info["backward"])
    print(f"{cfg}: tick / bare eval = " + " ".join(f"{r:.3f}" for r in out["device_over_bare"])
          + f"; best lockstep / worst device = {out['lockstep_best_over_device_worst']:.1f}; seed-ticks on done seeds "
          f"{out['device']['done_seed_tick_share']:.1%}", flush=True)
    return out


torch.cuda.set_device(0)
results = {cfg: run(cfg) for cfg in cfgs}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
path = os.path.join(ROOT, "profiles", f"bench_optimize_{TAG}.json")
with open(path, "w") as f:
    json.dump(results, f, indent=1)
print("wrote", path)
