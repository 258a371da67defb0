"""The envelope gradient's cost (diagnostic, plain timing): evals per second of qoc_eval_envelope_dev (J and dJ/dp, the
discrete Tsit5 adjoint) against qoc_propagate_envelope's forward alone, on
  drag         the 4-level transmon, m = 2, tgate 20, dt 0.01 (2000 steps), B = 512, np = 4
  tunable_bus  N = 27, m = 1, tgate 350, dt 1e-3 (350 000 steps), B = 64, np = 5
The yardstick is the only way to a gradient without the adjoint: central differences, 2 np forward calls (8 / 10).
Warm-up, then K timed calls between two synchronisations, 3 repeats, every repeat printed.  Each tree is timed in a
process of its own, one at a time; this driver never opens the GPU.
--parent DIR also times the forward of another checkout (built there: the parent commit, which has no eval) with
this tool, before this tree's.
Usage: python tools/bench_envelope.py [drag|tunable_bus ...] [--steps K] [--parent DIR]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 3


def opt(args, name, default, conv=str):
    if name in args:
        i = args.index(name)
        v = conv(args[i + 1])
        del args[i:i + 2]
        return v
    return default


def setup(case):
    import numpy as np
    from qoc_amd import systems as S
    if case == "drag":
        a = S.annihilation_op(4)
        ad = a.conj().T
        A0 = -1j * (-0.3 / 2) * (ad @ ad @ a @ a)
        A = [-1j * (a + ad) / 2, -1j * (1j * (ad - a)) / 2]
        x0 = np.eye(4, dtype=complex)[:, :2]
        xt = np.eye(4, dtype=complex)[:, [1, 0]]
        B = 512
        rng = np.random.default_rng(0)
        P = np.column_stack([np.full(B, 20.0), np.full(B, 5.0), rng.uniform(0.1, 0.4, B), rng.uniform(-1, 1, B)])
        return A0, A, x0, xt, 2, P, 20.0, 0.01, 20
    H0, Hc, qb = S.tunable_bus_model()
    x0 = qb.columns(["110"])[:, 0].astype(complex)
    xt = qb.columns(["200"])[:, 0].astype(complex)
    i1, i2 = int(np.argmax(np.abs(x0))), int(np.argmax(np.abs(xt)))
    w = abs(H0[i1, i1] - H0[i2, i2]) + (-0.002) * 2 * np.pi
    B = 64
    rng = np.random.default_rng(0)
    P = np.column_stack([rng.uniform(280, 320, B), rng.uniform(20, 60, B), rng.uniform(0.22, 0.27, B),
                         w * rng.uniform(0.99, 1.01, B), rng.uniform(0.10, 0.15, B)])
    return -1j * H0, [-1j * Hc], x0, xt, 1, P, 350.0, 1e-3, 1


def child(tree, cases, K):
    """Times one tree in this process; prints one JSON line per (case, leg)."""
    sys.path.insert(0, os.path.join(tree, "quantumoptimalcontrol.jl_amd"))
    import numpy as np
    import torch
    from qoc_amd import GrapeEngine
    torch.cuda.set_device(0)
    for case in cases:
        A0, A, x0, xt, n, P, tgate, dt, k_default = setup(case)
        k = K or k_default
        B, npar = P.shape
        eng = GrapeEngine(A0, A, x0, 1, B=B)
        eng.set_cost_trace(xt, n)
        dP = torch.from_numpy(P).cuda()
        dJ = torch.zeros(B, dtype=torch.float64, device="cuda")
        dg = torch.zeros(B, npar, dtype=torch.float64, device="cuda")
        legs = [("forward", lambda: eng.propagate_envelope(case, P, tgate, dt))]
        if hasattr(eng, "eval_envelope_device"):
            legs.append(("eval_dev", lambda: eng.eval_envelope_device(case, dP.data_ptr(), npar, tgate, dt, dJ.data_ptr(),
                                                                      dg.data_ptr())))
        for name, step in legs:
            step()
            eng.synchronize()
            rates = []
            for _ in range(REPEATS):
                eng.synchronize()
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(k):
                    step()
                eng.synchronize()
                torch.cuda.synchronize()
                rates.append(B * k / (time.perf_counter() - t))
            print(json.dumps({"tree": tree, "case": case, "leg": name, "B": B, "np": npar, "calls": k,
                              "evals_per_s": rates, "J0": float(dJ[0].item()),
                              "g0_norm": float(torch.linalg.vector_norm(dg[0]).item())}), flush=True)
        eng.close()


def main():
    args = sys.argv[1:]
    if "--child" in args:
        tree = opt(args, "--child", HERE)
        K = opt(args, "--steps", 0, int)
        return child(tree, args, K)
    K = opt(args, "--steps", 0, int)
    parent = opt(args, "--parent", None)
    cases = args or ["drag", "tunable_bus"]
    rows = []
    for tree in ([os.path.abspath(parent)] if parent else []) + [HERE]:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(K)] + cases,
                             capture_output=True, text=True)
        sys.stderr.write(out.stderr[-2000:])
        if out.returncode:
            sys.exit(f"{tree}: exit {out.returncode}")
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                r["which"] = "parent" if tree != HERE else "tree"
                rows.append(r)
                print(f"{r['which']:6s} {r['case']:11s} {r['leg']:8s} calls={r['calls']} "
                      + " ".join(f"{v:.4g}" for v in r["evals_per_s"]) + " evals/s", flush=True)

    def med(which, case, leg):
        for r in rows:
            if (r["which"], r["case"], r["leg"]) == (which, case, leg):
                return sorted(r["evals_per_s"])[1], r["np"]
        return None, None
    for case in cases:
        ev, npar = med("tree", case, "eval_dev")
        fw, _ = med("tree", case, "forward")
        pf, _ = med("parent", case, "forward")
        line = f"{case}: eval / forward (cost, medians) = {fw / ev:.2f}; eval / (2 np = {2 * npar} forwards) = {fw / ev / (2 * npar):.3f}"
        if pf:
            line += (f"; against the parent's forward: {pf / ev:.2f} and {pf / ev / (2 * npar):.3f}; "
                     f"forward tree / parent = {fw / pf:.3f}")
        print(line, flush=True)


if __name__ == "__main__":
    main()
