"""The exact (Fréchet) gradient's cost on the segmented eval and on the interpolating block propagators (diagnostic,
plain timing): evals per second of the fused eval_device and of the split propagate + grape_sensitivity at
  order 3                       the default gradient (k_blkseg_eval, ORD 3; tunable_bus: k_blkp_grad)
  exact                         dUkdp_order = "exact" on the segmented kernel (ORD 0; tunable_bus: k_blkp_grad_exact)
  exact, QOC_BLKSEG_EXACT=0     the dense Fréchet path (x_k and λ_k rebuilt in HBM, one 2N x 2N block exponential per
                                slice and control; tunable_bus: QOC_BLKP_EXACT=0)
on
  zz           N = 9,  Nt = 500,  B = 512
  cavity       N = 40, Nt = 1000, B = 256
  tunable_bus  N = 27, Nt = 2000, B = 512 (blocks of 13 / 14 rows, one control); its exact legs also print the gradient
               kernel's own time per eval (phase "k_grad" of phase_times, a profiled pass after the timed ones).
  cavity_dense N = 40, Nt = 1000, B = 256 (no invariant blocks: the dense chains and the fused gradient kernels).  Its
               exact leg is the series on MFMA (k_grad_rr_xn / _xq / _xp), its third leg QOC_GRAD_EXACT_SERIES=0, the
               block exponentials; the legs on the series also print the gradient phase's own time per eval and the
               series' counters (exact_series_stats).  Not in the default set: name it.
Warm-up, then K timed steps between two synchronisations, 3 repeats, every repeat printed, one process at a time.
A library from before the segmented exact gradient ignores the switch: run from a checkout of that commit, the two exact
legs both time its dense path (the fourth leg of DESIGN.md's table).
The dense path is orders of magnitude slower; --dense-steps / --dense-warm shorten the legs that leave the segmented
path (each step there is long enough to time on its own), the segmented legs always run --steps and the full warm-up.
--tree DIR times the package of another checkout (built there) with this tool: a library from before the dense series
ignores QOC_GRAD_EXACT_SERIES and has no counters, so its exact legs both time the block exponentials.
Usage: python tools/bench_exact.py [zz|cavity|tunable_bus|cavity_dense ...] [--steps K] [--dense-steps K2]
       [--dense-warm W2] [--tree DIR]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    _i = sys.argv.index("--tree")
    ROOT = os.path.abspath(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from qoc_amd import GrapeEngine, systems  # noqa: E402


def opt(args, name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


args = sys.argv[1:]
K = max(200, opt(args, "--steps", 200))
K_DENSE = max(1, opt(args, "--dense-steps", K))
WARM, REPEATS = 20, 3
WARM_DENSE = max(1, opt(args, "--dense-warm", WARM))
cfgs = args or ["zz", "cavity", "tunable_bus"]


def setup(cfg):
    mk_prob, mk_u, B = systems.CONFIGS["zz_batch" if cfg == "zz" else cfg]
    return mk_prob(), mk_u(B, 0), B


def fast_path(cfg):  # (the switch that leaves it, what info()["backward"] reports on it)
    if cfg == "cavity_dense":  # info()["backward"] does not tell the series from the block exponentials: on_fast_path
        return ("QOC_GRAD_EXACT_SERIES", None)
    return ("QOC_BLKP_EXACT", "blocks_prop16") if cfg == "tunable_bus" else ("QOC_BLKSEG_EXACT", "segmented")


def on_fast_path(cfg, eng, order, info):
    """Whether the step just run stayed off the block exponentials (which get the short --dense-steps legs)."""
    if cfg != "cavity_dense":
        return info["backward"] == fast_path(cfg)[1]
    if order == 3:
        return True
    stats = getattr(eng, "exact_series_stats", None)
    return stats is not None and stats()["units"] > 0


def leg(cfg, prob, u, B, order, switch):
    var, fast = fast_path(cfg)
    if switch is None:
        os.environ.pop(var, None)
    else:
        os.environ[var] = switch
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    eng.set_cost_trace(prob.x_target, prob.n)
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device="cuda")

    def fused():
        eng.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())

    def split():
        eng.propagate_device(ud.data_ptr(), Jd.data_ptr())
        eng.grape_sensitivity_device(ud.data_ptr(), order, gd.data_ptr())

    out = {}
    tag = f"order {order}" if switch is None else f"order {order} {var}={switch}"
    for form, step in (("fused", fused), ("split", split)):
        step()
        eng.synchronize()
        info = eng.info()
        seg = on_fast_path(cfg, eng, order, info)
        warm, steps = (WARM, K) if seg else (WARM_DENSE, K_DENSE)
        for _ in range(warm - 1):
            step()
        eng.synchronize()
        rates = []
        for _ in range(REPEATS):
            eng.synchronize()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(steps):
                step()
            eng.synchronize()
            torch.cuda.synchronize()
            rates.append(B * steps / (time.perf_counter() - t))
        out[form] = rates
        gn = float(torch.linalg.vector_norm(gd[0]).item())
        print(f"{cfg} {form:5s} {tag:32s} backward={info['backward']} split_forward={info['split_forward']} "
              f"steps={steps} J[0]={Jd[0].item():.15g} |g[0]|={gn:.15g} "
              + " ".join(f"{r / 1e6:.6f}" for r in rates) + " M evals/s", flush=True)
        if cfg == "cavity_dense" and seg and order != 3:
            print(f"{cfg} {form:5s} {tag:32s} exact_series_stats after {warm + REPEATS * steps} steps: "
                  f"{eng.exact_series_stats(reset=True)}", flush=True)
        if cfg in ("tunable_bus", "cavity_dense") and seg:  # the gradient kernel's own time, from events around its launches
            eng.set_profiling(True)
            eng.phase_times(reset=True)
            for _ in range(10):
                step()
            eng.synchronize()
            pt = eng.phase_times(reset=True)
            eng.set_profiling(False)
            print(f"{cfg} {form:5s} {tag:32s} per eval of {B} seeds: "
                  + " ".join(f"{k} {ms / 10:.3f} ms ({n // 10} launches)" for k, (ms, n) in pt.items()), flush=True)
    eng.close()
    return out


torch.cuda.set_device(0)
for cfg in cfgs:
    prob, u, B = setup(cfg)
    o3 = leg(cfg, prob, u, B, 3, None)
    ex = leg(cfg, prob, u, B, "exact", None)
    dn = leg(cfg, prob, u, B, "exact", "0")
    for form in ("fused", "split"):
        print(f"{cfg} {form}: exact / order 3 (medians) = {np.median(ex[form]) / np.median(o3[form]):.3f}; "
              f"worst exact repeat / best {fast_path(cfg)[0]}=0 repeat = {min(ex[form]) / max(dn[form]):.1f}", flush=True)
    os.environ.pop(fast_path(cfg)[0], None)
