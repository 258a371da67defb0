"""Robust-control evals (diagnostic, plain timing): (pulse, member) evals per second of one eval of B pulses over an
ensemble of E generator sets, as
  ensemble   one context with set_generator_ensemble: one launch of B E workgroups and the reduction launch;
             where B E >= 2048 also with QOC_BLKSEG_W = 2 and 4 (the sweep that set the shape rule's floor of 4 waves
             for ensemble launches, DESIGN.md §5 "Ensemble evals"; the plain rule would give one wave there)
  contexts   what a caller can do without it: E contexts (one per member, each with a stream of its own), eval_device
             on each with the same u, and the weighted sums in torch on the first context's stream, ordered by events
             (no host synchronisation between the steps)
on
  cavity  N = 40, Nt = 1000  (20 blocks of 2; detuning ±2e-3 and amplitude ±4 % spread over the members)
  zz      N = 9,  Nt = 500   (3 blocks of 3; ZZ strength and one anharmonicity spread over the members)
at (B, E) = (32, 8) and (256, 8), order 3 and exact.  Warm-up of 20 steps, then K = 200 timed steps between two
synchronisations, 3 repeats, every repeat printed, one process at a time.
--parent DIR times the package of another checkout (built there) with this tool: a library from before the ensemble
has the contexts leg only.
Usage: python tools/bench_ensemble.py [cavity|zz ...] [--steps K] [--parent DIR]"""
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
    K = max(200, int(args[_i + 1]))
    del args[_i:_i + 2]
WARM, REPEATS = 20, 3
SHAPES = ((32, 8), (256, 8))
cfgs = args or ["cavity", "zz"]
HAS_ENS = hasattr(GrapeEngine, "set_generator_ensemble")


def members(cfg, prob, E):
    """(A0s (E, N, N), As [nu x (E, N, N)]): the spreads of the module docstring, member e at fraction e / (E - 1)."""
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
    N = prob.N
    A0s = np.stack([prob.A0 + d for d in dA0])
    As = [np.stack([np.asarray(A) * s for s in amp]) for A in prob.A]
    assert A0s.shape == (E, N, N)
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


def show(cfg, B, E, order, leg, rates, extra=""):
    print(f"{cfg} B={B} E={E} order {order} {leg:14s} " + " ".join(f"{r / 1e6:.6f}" for r in rates)
          + f" M (pulse, member) evals/s{extra}", flush=True)


def leg_ensemble(cfg, prob, u, A0s, As, w, order, W):
    if W is None:
        os.environ.pop("QOC_BLKSEG_W", None)
    else:
        os.environ["QOC_BLKSEG_W"] = str(W)
    B, E = u.shape[0], A0s.shape[0]
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    eng.set_cost_trace(prob.x_target, prob.n)
    eng.set_generator_ensemble(A0s, As, w)
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
    out = Jd[0].item(), float(torch.linalg.vector_norm(gd[0]).item())
    eng.close()
    os.environ.pop("QOC_BLKSEG_W", None)
    return rates, out


def leg_contexts(cfg, prob, u, A0s, As, w, order):
    B, E = u.shape[0], A0s.shape[0]
    engs = []
    for e in range(E):
        eng = GrapeEngine(A0s[e], [a[e] for a in As], prob.x0, prob.Nt, B=B)
        eng.set_cost_trace(prob.x_target, prob.n)
        engs.append(eng)
    streams = [torch.cuda.ExternalStream(eng.stream()) for eng in engs]
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    Jm = torch.empty(E, B, dtype=torch.float64, device="cuda")
    gm = torch.empty(E, B, prob.Nt, prob.nu, dtype=torch.float64, device="cuda")
    wd = torch.tensor(w, dtype=torch.float64, device="cuda")
    res = {}
    torch.cuda.synchronize()
    summed = [None]

    def step():
        for e in range(E):
            if summed[0] is not None and e > 0:
                streams[e].wait_event(summed[0])  # the last step's sums have read this member's buffers
            engs[e].eval_device(ud.data_ptr(), order, Jm[e].data_ptr(), gm[e].data_ptr())
            if e > 0:
                streams[0].wait_event(streams[e].record_event())
        with torch.cuda.stream(streams[0]):
            res["J"] = torch.tensordot(wd, Jm, dims=1)
            res["g"] = torch.tensordot(wd, gm, dims=1)
        summed[0] = streams[0].record_event()

    def sync():
        for eng in engs:
            eng.synchronize()
        torch.cuda.synchronize()
    rates = timed(step, sync, B * E)
    out = res["J"][0].item(), float(torch.linalg.vector_norm(res["g"][0]).item())
    for eng in engs:
        eng.close()
    return rates, out


torch.cuda.set_device(0)
for cfg in cfgs:
    mk_prob, mk_u, _ = systems.CONFIGS["zz_batch" if cfg == "zz" else cfg]
    prob = mk_prob()
    for B, E in SHAPES:
        u = mk_u(B, 0)
        A0s, As = members(cfg, prob, E)
        w = np.full(E, 1.0 / E)
        for order in (3, "exact"):
            med = {}
            if HAS_ENS:
                for W in (None, 2, 4) if B * E >= 2048 else (None,):
                    leg = "ensemble" if W is None else f"ensemble W={W}"
                    rates, out = leg_ensemble(cfg, prob, u, A0s, As, w, order, W)
                    show(cfg, B, E, order, leg, rates, f"  J[0]={out[0]:.15g} |g[0]|={out[1]:.15g}")
                    med[leg] = float(np.median(rates))
            rates, out = leg_contexts(cfg, prob, u, A0s, As, w, order)
            show(cfg, B, E, order, "contexts", rates, f"  J[0]={out[0]:.15g} |g[0]|={out[1]:.15g}")
            med["contexts"] = float(np.median(rates))
            if HAS_ENS:
                print(f"{cfg} B={B} E={E} order {order}: ensemble / contexts (medians) = "
                      + ", ".join(f"{k}: {v / med['contexts']:.3f}" for k, v in med.items() if k != "contexts"),
                      flush=True)
