"""Gate-duration evals (diagnostic, plain timing), in evals per second:
  flag    what the TS kernels cost: eval_device with set_time_scale(1 for every seed) against the plain eval of the
          same build, on two contexts whose timed repeats alternate (plain, scaled, plain, scaled, ...);
          cavity (N = 40, Nt = 1000, B = 256) and zz (N = 9, Nt = 500, B = 512), with and without the state penalty,
          order 3 and exact
  sweep   what a gate-time sweep gains: 16 durations x 16 seeds in one context (B = 256, set_time_scale) against the
          caller's form without it, 16 contexts of B = 16 with τ-scaled generators evaluated back to back (each waits
          for the one before it through an event: one stream's order), cavity and zz, order 3
Warm-up of 20 steps, then K = 200 timed steps between two synchronisations, 3 repeats, every repeat printed, one
process at a time.
--parent DIR times the package of another checkout (built there) with this tool: a library from before the time scale
has the plain and the contexts legs only.
Usage: python tools/bench_duration.py [flag|sweep ...] [--steps K] [--parent DIR]"""
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


torch.cuda.set_device(0)
for p in parts:
    {"flag": part_flag, "sweep": part_sweep}[p]()
