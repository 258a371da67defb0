"""Ensemble objectives (diagnostic, plain timing): (pulse, member) evals per second of one eval of B pulses over an
ensemble of E = 8 generator sets under CVaR with uniform weights 1/8 and α = n / 8, so that exactly n = n_act members
carry weight (n = 1 is the worst case), as
  route 2   QOC_ENS_SKIP=1: the forward half for every (pulse, member), k_ens_weights, the backward half where ω is not
            0, k_ens_reduce_w
  route 1   QOC_ENS_SKIP=0: the fused launch for every (pulse, member), k_ens_weights, k_ens_reduce_w
and the MEAN leg (the default objective: the fused launch and k_ens_reduce), on
  cavity  N = 40, Nt = 1000  (20 blocks of 2)
  zz      N = 9,  Nt = 500   (3 blocks of 3)
at (B, E) = (32, 8) and (256, 8), order 3 and exact.  Warm-up of 20 steps, then K = 200 timed steps between two
synchronisations, 3 repeats, every repeat printed, one process at a time.  These are the sweeps that set the route rule
(csrc/qoc_run_blkseg.hip ENS_SKIP_TAU and ENS_SKIP_WG_PER_CU; DESIGN.md §5 "Ensemble objectives"): τ is the largest
n / E at which route 2 wins every repeat on both configs, among the shapes with enough workgroups per compute unit
for it to win at all.
--shapes 64x8,128x8,512x8 times other (B, E) and --nmax N stops the sweep at n = N (the sweep between the two shapes);
--mean-only times the MEAN leg alone; --parent DIR times the package of another checkout (built there) with this tool:
a library from before the objectives has the MEAN leg only, which is the same code path.
Usage: python tools/bench_ensemble_risk.py [cavity|zz ...] [--steps K] [--shapes BxE,...] [--nmax N] [--mean-only]
       [--parent DIR]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "head"
if "--parent" in sys.argv:
    _i = sys.argv.index("--parent")
    ROOT = os.path.abspath(sys.argv[_i + 1])
    TAG = "parent"
    del sys.argv[_i:_i + 2]
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from qoc_amd import GrapeEngine, systems  # noqa: E402

args = sys.argv[1:]
K = 200
if "--steps" in args:
    _i = args.index("--steps")
    K = max(200, int(args[_i + 1]))
    del args[_i:_i + 2]
SHAPES = ((32, 8), (256, 8))
NMAX = None
if "--shapes" in args:
    _i = args.index("--shapes")
    SHAPES = tuple(tuple(int(x) for x in t.split("x")) for t in args[_i + 1].split(","))
    del args[_i:_i + 2]
if "--nmax" in args:
    _i = args.index("--nmax")
    NMAX = int(args[_i + 1])
    del args[_i:_i + 2]
MEAN_ONLY = "--mean-only" in args
args = [a for a in args if a != "--mean-only"]
WARM, REPEATS = 20, 3
cfgs = args or ["cavity", "zz"]
HAS_OBJ = hasattr(GrapeEngine, "set_ensemble_objective")


def members(cfg, prob, E):
    """tools/bench_ensemble.py's spreads: member e at fraction e / (E - 1) of detuning ±2e-3 and amplitude ±4 % (cavity),
    of the ZZ strength and one anharmonicity (zz)."""
    t = np.linspace(-1.0, 1.0, E)
    if cfg == "cavity":
        b = systems.annihilation_op(2)
        D = -1j * np.kron(b.T @ b, np.eye(prob.N // 2))
        dA0, amp = [2e-3 * x * D for x in t], [1.0 + 0.04 * x for x in t]
    else:
        a = systems.annihilation_op(3)
        n = a.T @ a
        dt = 20.0 / prob.Nt
        Hint = -2 * np.pi * 1e-4 * np.kron(n, n)
        Hq = -2 * np.pi * 0.2 / 2 * np.kron(a.T @ a.T @ a @ a, np.eye(3))
        dA0, amp = [-1j * dt * (0.5 * x * Hint + 0.03 * x * Hq) for x in t], [1.0] * E
    A0s = np.stack([prob.A0 + d for d in dA0])
    As = [np.stack([np.asarray(A) * s for s in amp]) for A in prob.A]
    return A0s, As


def timed(step, sync, units):
    for _ in range(WARM):
        step()
    sync()
    rates = []
    for _ in range(REPEATS):
        sync()
        t = time.perf_counter()
        for _ in range(K):
            step()
        sync()
        rates.append(units * K / (time.perf_counter() - t))
    return rates


def leg(prob, u, A0s, As, w, order, kind, param, skip):
    """One engine, one objective, one forced route -> rates, (J̄[0], |dJ̄/du[0]|, route, active members of pulse 0)."""
    B, E = u.shape[0], A0s.shape[0]
    if skip is None:
        os.environ.pop("QOC_ENS_SKIP", None)
    else:
        os.environ["QOC_ENS_SKIP"] = str(skip)
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    eng.set_cost_trace(prob.x_target, prob.n)
    eng.set_generator_ensemble(A0s, As, w)
    if kind != "mean":
        eng.set_ensemble_objective(kind, param)
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def step():
        eng.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())

    def sync():
        eng.synchronize()
        torch.cuda.synchronize()
    rates = timed(step, sync, B * E)
    route = eng.ensemble_objective[2] if HAS_OBJ else 1
    act = int(np.count_nonzero(eng.member_weights()[0])) if HAS_OBJ else E
    out = Jd[0].item(), float(torch.linalg.vector_norm(gd[0]).item()), route, act
    eng.close()
    os.environ.pop("QOC_ENS_SKIP", None)
    return rates, out


def show(cfg, B, E, order, name, rates, out):
    print(f"{TAG} {cfg} B={B} E={E} order {order} {name:16s} " + " ".join(f"{r / 1e6:.6f}" for r in rates)
          + f" M (pulse, member) evals/s  route {out[2]} active {out[3]} J[0]={out[0]:.15g} |g[0]|={out[1]:.15g}",
          flush=True)


torch.cuda.set_device(0)
wins = {}
for cfg in cfgs:
    mk_prob, mk_u, _ = systems.CONFIGS["zz_batch" if cfg == "zz" else cfg]
    prob = mk_prob()
    for B, E in SHAPES:
        u = mk_u(B, 0)
        A0s, As = members(cfg, prob, E)
        w = np.full(E, 1.0 / E)
        for order in (3, "exact"):
            rates, out = leg(prob, u, A0s, As, w, order, "mean", None, None)
            show(cfg, B, E, order, "mean", rates, out)
            if MEAN_ONLY or not HAS_OBJ:
                continue
            for n in range(1, min(E, NMAX or E) + 1):
                r2, o2 = leg(prob, u, A0s, As, w, order, "cvar", n / E, 1)
                r1, o1 = leg(prob, u, A0s, As, w, order, "cvar", n / E, 0)
                assert o2[2] == 2 and o1[2] == 1 and o2[3] == n and o1[:2] == o2[:2], (o1, o2)
                show(cfg, B, E, order, f"cvar n={n} route 2", r2, o2)
                show(cfg, B, E, order, f"cvar n={n} route 1", r1, o1)
                won = min(r2) > max(r1)
                wins.setdefault(n, []).append(won)
                print(f"{TAG} {cfg} B={B} E={E} order {order} n={n}: route 2 / route 1 (medians) = "
                      f"{np.median(r2) / np.median(r1):.3f}, route 2 / mean = {np.median(r2) / np.median(rates):.3f}, "
                      f"route 2 wins every repeat: {won}", flush=True)
if wins:
    ok = [n for n in sorted(wins) if all(all(wins[k]) for k in range(1, n + 1))]
    print(f"route 2 wins every repeat on every config and shape up to n_act = {max(ok) if ok else 0}", flush=True)
