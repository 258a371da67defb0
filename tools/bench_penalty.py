"""The guard-state penalty's cost (diagnostic, plain timing): evals per second of the fused eval_device and of the split
propagate + grape_sensitivity, unpenalised, penalised on the config's fast path, and penalised with that path's switch
off (the block chains' fallback), on
  zz              N = 9,  Nt = 500,  B = 512, P = |20>, |21>, |22>, C = 0..3, mu = 1e-9 dt / tgate
                  (examples/zz_coupling_ipopt_exp.jl:42-46); segmented eval, QOC_BLKSEG_PEN
  cavity          N = 40, Nt = 1000, B = 256, P = the top two cavity levels of both qubit states, C = 0..1, the same mu
                  rule; segmented eval, QOC_BLKSEG_PEN
  tunable_bus     N = 27, Nt = 2000, B = 512, m = 1, P = |020>, |011>, |002>, |101> (the even block's guard states),
                  C = 0; interpolating block propagators, QOC_BLKP_PEN
  tunable_bus_cz  the same model as a CZ gate, m = 4, B = 256, P = |200>, |020>, |002>, |110>, |011>, C = 0..3; stored
                  block propagators, QOC_BLKP_PEN
Warm-up, then K timed steps between two synchronisations, 3 repeats, every repeat printed.  A library without the
switch ignores it: there the last two legs both time that library's penalised path.
Usage: python tools/bench_penalty.py [zz|cavity|tunable_bus|tunable_bus_cz ...] [--steps K]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from qoc_amd import GrapeEngine, systems  # noqa: E402

args = sys.argv[1:]
K = 200
if "--steps" in args:
    i = args.index("--steps")
    K = max(200, int(args[i + 1]))
    del args[i:i + 2]
cfgs = args or ["zz", "cavity"]
WARM, REPEATS = 20, 3


SWITCH = {"zz": "QOC_BLKSEG_PEN", "cavity": "QOC_BLKSEG_PEN", "tunable_bus": "QOC_BLKP_PEN",
          "tunable_bus_cz": "QOC_BLKP_PEN"}


def setup(cfg):
    if cfg in ("tunable_bus", "tunable_bus_cz"):
        qb = systems.QuantumBasis([3, 3, 3])
        if cfg == "tunable_bus":
            prob, B = systems.tunable_bus_problem(2000), 512
            pen = ([int(r) for r in qb(["020", "011", "002", "101"])], [0], 1e-9 / prob.Nt)
        else:
            prob, B = systems.tunable_bus_cz_problem(2000), 256
            pen = ([int(r) for r in qb(["200", "020", "002", "110", "011"])], [0, 1, 2, 3], 1e-9 / prob.Nt)
        return prob, systems.tunable_bus_controls(B, prob.Nt, 0), B, pen
    if cfg == "zz":
        mk_prob, mk_u, B = systems.CONFIGS["zz_batch"]
        prob = mk_prob()
        qb = systems.QuantumBasis([3, 3])
        pen = ([int(r) for r in qb(["20", "21", "22"])], [0, 1, 2, 3], 1e-9 / prob.Nt)
    else:
        mk_prob, mk_u, B = systems.CONFIGS["cavity"]
        prob = mk_prob()
        nc = prob.N // 2  # qubit first: row q nc + n
        pen = ([nc - 2, nc - 1, 2 * nc - 2, 2 * nc - 1], [0, 1], 1e-9 / prob.Nt)
    return prob, mk_u(B, 0), B, pen


def leg(cfg, prob, u, B, pen, switch):
    if switch is None:
        os.environ.pop(SWITCH[cfg], None)
    else:
        os.environ[SWITCH[cfg]] = switch
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    eng.set_cost_trace(prob.x_target, prob.n)
    if pen is not None:
        eng.set_state_penalty(*pen)
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device="cuda")

    def fused():
        eng.eval_device(ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())

    def split():
        eng.propagate_device(ud.data_ptr(), Jd.data_ptr())
        eng.grape_sensitivity_device(ud.data_ptr(), 3, gd.data_ptr())

    out = {}
    for form, step in (("fused", fused), ("split", split)):
        for _ in range(WARM):
            step()
        eng.synchronize()
        info = eng.info()
        rates = []
        for _ in range(REPEATS):
            eng.synchronize()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(K):
                step()
            eng.synchronize()
            torch.cuda.synchronize()
            rates.append(B * K / (time.perf_counter() - t))
        out[form] = rates
        tag = "unpenalised" if pen is None else "penalised" if switch is None else f"penalised {SWITCH[cfg]}=0"
        print(f"{cfg} {form:5s} {tag:27s} backward={info['backward']} split_forward={info['split_forward']} J[0]={Jd[0].item():.15g} "
              + " ".join(f"{r / 1e6:.4f}" for r in rates) + " M evals/s", flush=True)
    eng.close()
    return out


torch.cuda.set_device(0)
for cfg in cfgs:
    prob, u, B, pen = setup(cfg)
    base = leg(cfg, prob, u, B, None, None)
    new = leg(cfg, prob, u, B, pen, None)
    leg(cfg, prob, u, B, pen, "0")
    for form in ("fused", "split"):
        print(f"{cfg} {form}: penalised / unpenalised (medians) = {np.median(new[form]) / np.median(base[form]):.3f}",
              flush=True)
    os.environ.pop(SWITCH[cfg], None)
