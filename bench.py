#!/usr/bin/env python
"""bench.py — GRAPE gradient evals/sec on MI355X (BASELINE.json metric).

One *step* = one GRAPE gradient eval of every seed resident on this GPU:
propagate (exponentials + forward chain + trace cost) + grape_sensitivity
(order-3 Taylor Jacobian contraction + co-state chain) — Ipopt's f + f_grad of
examples/ipopt_callbacks_exp.jl:11-31 without the spline map.  Inputs (u) are resident
in HBM before the timed region.  Seeds are sharded across ranks (weak scaling); the only
collective is the RCCL all-gather of each rank's best (J, seed) per step.

Run:  python bench.py [--gpus N --steps K --warmup W --config cavity --call-form fused] [--full] [--dump-outputs DIR]
      python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run sets up, warms up, times the K steps and prints the result line (with the roofline figures of the timed steps'
own phase events).  --full adds what runs beside the metric: the CPU baseline and the parity check against it, and the
side legs (the other configs and the split call form).  --dump-outputs DIR writes what the last timed step returned
(J, dJdu or dJdc, best) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.

--call-form: "fused" (default) one device call per eval (qoc_eval_dev); "split" the reference's own call form,
qoc_propagate_dev then qoc_grape_sensitivity_dev (Ipopt's f then f_grad, examples/ipopt_callbacks_exp.jl:11-31) on the
same HBM-resident u; "ipopt" the Julia shim's callbacks verbatim: qoc_propagate_spline then qoc_sensitivity_spline with
host spline coefficients (10 B-splines per control, PCIe and both host syncs inside the timed region: a latency figure,
not the contract's resident-input rate).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "quantumoptimalcontrol.jl_amd"))

# MI355X dense peaks (MI355X_MICROARCH.md chip table; fp64 matrix = fp64 vector = 78.6 TF spec).
PEAK_TFLOPS = {"fp64": 78.6, "fp32": 157.3}
PEAK_HBM_GBS = 8000.0
GEMMS_PER_DEGREE = {3: 2, 5: 3, 7: 4, 9: 5, 13: 6}

WORKLOADS = {
    "cavity": "cavity_qubit: cavity(20) x qubit(2) dim N=40, m=2, nu=2, Nt=1000, B=256 seeds/GPU, order-3 gradient",
    "cavity_dense": ("cavity_qubit with the drive also displacing the cavity (Tc = b^dag x I + I x a^dag: no invariant "
                     "blocks, dense chains): dim N=40, m=2, nu=2, Nt=1000, B=256 seeds/GPU, order-3 gradient"),
    "zz_batch": "zz_coupling: dim N=9, m=4, nu=2, Nt=500, B=512 seeds/GPU, order-3 gradient",
    "tunable_bus": "two_qubit_tunable_bus: dim N=27, m=1, nu=1, Nt=2000, B=512 seeds/GPU, order-3 gradient",
    "zz_plumbing": "zz_coupling Ipopt plumbing: dim N=9, m=4, nu=2, Nt=100, B=1, order-3 gradient",
    "synthetic": ("synthetic GUE H0/Hc: dim N=256, m=256 (x0=I), nu=2, Nt=1000, B=128 seeds/GPU, fp32, "
                  "order-3 gradient (large-N batched-GEMM path)"),
}


def expm_flops(N, hist):
    """Algorithmic FLOPs of Padé exponentials (degree-minimal GEMMs + LU solve) for a (d, s) histogram."""
    return sum(cnt * (8.0 * N ** 3 * (GEMMS_PER_DEGREE[d] + s) + (40.0 / 3.0) * N ** 3) for (d, s), cnt in hist.items())


def taylor_gemms(m, large=False):
    """Complex GEMMs of one executed Taylor polynomial: m = 12 is the 4-product scheme (A2, A3, B4^2,
    (B2 + A6) A6); on the large-N path m = 8 is the 3-product scheme (A2, A2 P, L R); otherwise m = 3r+2 is
    Paterson-Stockmeyer (A2, A3, r Horner products in A3)."""
    if m == 12:
        return 4
    if m == "8t":
        return 3
    return 2 + (m - 2) // 3


def taylor_flops(N, thist, large=False):
    """Algorithmic FLOPs of the executed Taylor exponentials: taylor_gemms(m) + s squarings, 8 N^3 each."""
    return sum(cnt * 8.0 * N ** 3 * (taylor_gemms(m, large) + s) for (m, s), cnt in thist.items())


def ref_eval_flops(N, m, nu, hist_per_eval, order=3):
    """Reference-equivalent FLOPs of one eval (SURVEY.md §8d F_eval) for the measured (d, s) mix."""
    gj = {1: 0, 2: 2, 3: 5, 4: 9}[order] * nu + (1 if order == 4 else 0)
    nslices = sum(hist_per_eval.values())
    f = expm_flops(N, hist_per_eval)
    f += nslices * (8.0 * N ** 2 * m + 8.0 * N ** 2 * m + 8.0 * N ** 3 * gj + 8.0 * N ** 2 * m * nu)
    return f


def grad_flops(N, m, nu, Nt, B, order, captured=False):
    """Executed algorithmic FLOPs of the gradient phase.  Order 3 (the Ipopt path): 4 generator-combine products
    (N x (nu+1)N per state column: P1, P2, Q1, Q2) and 3 nu contraction products (A_j P_a), 8 N^2 m each per slice;
    with the chains' captured products (k_grad_rr_c) P1, P2, Q1, Q2 come from the chains and only the 3 nu
    contractions run.  Other orders: k_grad's (order-1) X and X^H matvecs + nu*order A_j matvecs."""
    mv = 8.0 * N * N * m
    if order == 3:
        return B * Nt * mv * ((0 if captured else 4 * (nu + 1)) + 3 * nu)
    return B * Nt * (2 * (order - 1) * mv + nu * order * mv)


def block_sizes(prob):
    """Row counts of the generators' invariant blocks (connected components of the union sparsity pattern of
    A_0..A_nu), as the engine's qoc_set_generators finds them for the block chains (csrc/qoc_blk.hpp)."""
    import numpy as np
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    M = np.abs(np.asarray(prob.A0)) > 0
    for a in prob.A:
        M |= np.abs(np.asarray(a)) > 0
    _, lab = connected_components(csr_matrix(M), directed=False)
    return np.bincount(lab)


def live_block_sizes(prob):
    """Row counts of the invariant blocks that carry state: x0 or X_target nonzero on some row of the block.  The
    concurrent eval gives blocks of 5..16 rows without state no chain waves (qoc_run_blk.hip blk_live; the tunable
    bus' odd-parity block at m = 1), so their work is not counted."""
    import numpy as np
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    M = np.abs(np.asarray(prob.A0)) > 0
    for a in prob.A:
        M |= np.abs(np.asarray(a)) > 0
    nb, lab = connected_components(csr_matrix(M), directed=False)
    rows = (np.abs(np.asarray(prob.x0)).sum(axis=1) > 0) | (np.abs(np.asarray(prob.x_target)).sum(axis=1) > 0)
    sizes = np.bincount(lab, minlength=nb)
    live = np.bincount(lab, weights=rows.astype(np.float64), minlength=nb) > 0
    return sizes[live] if live.any() else sizes


def blkseg_series_k(prob, u_all):
    """Per seed, the closed-form series degree K the segmented eval picks for blocks of 2 rows (qoc_blkseg.hpp
    blkseg_series_k): from ρ = ρ_0 + max_k Σ_j |u_jk| ρ_j with ρ_j the spectral half-width of the generator (the
    engine adds a small backward-error margin to ρ_j, which can move a seed at a class edge)."""
    import numpy as np
    rad = []
    for A in [prob.A0] + list(prob.A):
        ev = np.linalg.eigvalsh(1j * np.asarray(A))
        rad.append(0.5 * (ev.max() - ev.min()))
    rho = rad[0] + np.max(np.einsum("bjk,j->bk", np.abs(u_all), np.asarray(rad[1:])), axis=1)
    return np.where(rho <= 0.24, 5, np.where(rho <= 0.66, 7, 9))


def blkseg_unit_flops(nb, order, P=None, K=9, zd=False):
    """Executed fp64 flops of the segmented block eval (csrc/qoc_blkseg.hpp) per (slice, block) unit, counted from
    the kernel's code (FMA = 2, add / mul = 1), phase 1 and phase 3 (the block exponential is formed in both: it is
    recomputed, not stored).  Blocks of 2 rows (the skew-Hermitian fast path): closed-form exponential (Â 16, the
    cos / sinc series of degree 2K + 1 in omega^2 and t^2 8 (K + 1): 80 at K = 9, the rest 41), 2x2 complex products
    64 each, the
    contraction in the Pauli basis (sk2_contract_pauli) 20 / 53 / 75 at orders 1 / 2 / 3, 16 + 104 (order - 1) on
    skew X at order 4 (sk2_contract); blocks of 3 rows: the Taylor polynomial of degree P in the
    Cayley-Hamilton basis (478 + 26 (P + 1)), 3x3 products 216 each, the contraction 86 + 518 (order - 1).
    zd (blocks of 2 rows; control generators with zero diagonals and zero shifts, qoc_blkseg.hpp ZD): the block's
    diagonal, its half-difference and the phase series cos t, sin t are the same in every slice and computed once per
    lane, so the exponential takes 43 + 4 (K + 1) flops, phase 3's μ_k 0 and the Pauli contraction's x0, x3, x0² none."""
    if nb == 2:
        form = (43.0 + 4.0 * (K + 1)) if zd else (57.0 + 8.0 * (K + 1))
        prod = 64.0
        contr = {1: 20.0, 2: 53.0, 3: 75.0}.get(order, 16.0 + 104.0 * (order - 1))
        if zd and order in (2, 3):
            contr -= 4.0 if order == 2 else 5.0
        return form + prod, form + 2 * prod + (2.0 if zd else 6.0) + contr + 2.0
    form = 478.0 + 26.0 * ((P or 8) + 1)
    prod, contr = 216.0, 86.0 + 518.0 * (order - 1)
    return form + prod, form + 2 * prod + 76.0 + contr + 2.0


def blkseg_segments(B, Nt, nblk, ncu=256):
    """Segments per seed of the segmented eval (qoc_run_blk.hip blkseg_shape): 8 waves per CU shared by the seeds a CU
    holds, 64 / nblk segments per wave, then trimmed so that no segment is empty."""
    per_cu = max(1, min(8, -(-B // ncu)))
    S = max(1, min(max(1, 8 // per_cu) * (64 // max(1, nblk)), Nt))
    L = -(-Nt // S)
    return -(-Nt // L)


def chain_bytes(N, m, Nt, B, esz):
    """Compulsory HBM bytes of one chain launch: read all U_k once, write the N x m state per slice."""
    return B * Nt * N * N * esz + B * (Nt + 1) * N * m * esz


def cpu_baseline_large(prob, u_all, order, nthreads, target_s=12.0):
    """Large N: the numpy/OpenBLAS restatement (oracle/qoc_oracle.py; zgemm + LAPACK gesv, i.e. the
    reference's own BLAS/LAPACK call structure) on one seed and a bounded prefix of its slices;
    per-eval time = per-slice time x Nt (every slice does the same work)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import qoc_oracle as O  # checker / baseline only (oracle/)
    Nt = u_all.shape[2]
    n1 = 2
    t = time.perf_counter()
    O.grape_eval(prob.A0, prob.A, u_all[0, :, :n1], prob.x0, prob.x_target, prob.n, order=order)
    t1 = (time.perf_counter() - t) / n1
    n2 = int(max(2, min(Nt, target_s / max(t1, 1e-4))))
    t = time.perf_counter()
    Jc, gc, _ = O.grape_eval(prob.A0, prob.A, u_all[0, :, :n2], prob.x0, prob.x_target, prob.n, order=order)
    t2 = time.perf_counter() - t
    per_eval = t2 / n2 * Nt
    return {
        "value": 1.0 / per_eval,
        "unit": "evals/s",
        "cores": nthreads,
        "kind": "port",
        "sample": (f"oracle/qoc_oracle.py (numpy + OpenBLAS zgemm/LAPACK gesv, {nthreads} BLAS threads) on "
                   f"seed 0, first {n2} of {Nt} slices in {t2:.1f} s; evals/s = 1/(per-slice time x {Nt})"),
    }, (Jc, gc, n2)


def cpu_facts():
    """CPU model, visible / usable cores (the box's nproc counts the whole machine; the job's share is its
    affinity mask and OMP_NUM_THREADS)."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count() or 1
    return model, os.cpu_count() or 1, aff


def cpu_threads():
    """Threads for the CPU baseline: the job's CPU share (OMP_NUM_THREADS, set by the launcher to the cores
    allotted to one GPU), else every core in the affinity mask."""
    _, _, aff = cpu_facts()
    env = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return min(env, aff) if env > 0 else aff


def cpu_baseline(prob, u_all, order, nthreads, target_s=12.0):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpuref  # checker / baseline only (oracle/)
    import numpy as np
    model, ncpu, aff = cpu_facts()
    B = u_all.shape[0]
    # calibration round (one seed per thread, seed-parallel) for both backends of the port: zgemm / zgesv from
    # the image's OpenBLAS (the reference runs MKL's) and the in-repo loops; OpenBLAS pays a per-call overhead
    # at small N and contends when many threads call it at once, so the faster backend is timed
    S = min(B, nthreads)
    calib = {}
    for use in (True, False):
        path = cpuref.use_blas(use)
        if use and not path:
            continue
        t = time.perf_counter()
        cpuref.grape_eval_batch(prob, u_all[:S], order=order, mode=0, nthreads=nthreads)
        calib[path] = time.perf_counter() - t
    blas = min(calib, key=calib.get)
    cpuref.use_blas(blas is not None)
    t1 = calib[blas]
    # timed sample: ~target_s of CPU work, i.e. `total` evals over the first S2 seeds (repeated passes
    # when the batch has fewer seeds than that)
    total = int(max(S, S * round(target_s / max(t1, 1e-3))))
    S2 = min(B, total)
    t = time.perf_counter()
    J, g = cpuref.grape_eval_batch(prob, u_all[:S2], order=order, mode=0, nthreads=nthreads)
    done = S2
    while done < total:
        n = min(S2, total - done)
        cpuref.grape_eval_batch(prob, u_all[:n], order=order, mode=0, nthreads=nthreads)
        done += n
    t2 = time.perf_counter() - t
    seed_par = done / t2
    # reference-faithful mode (exponentials parallel over k, seeds one after another): 1 seed
    t = time.perf_counter()
    cpuref.grape_eval_batch(prob, u_all[:1], order=order, mode=1, nthreads=nthreads)
    faithful = 1.0 / (time.perf_counter() - t)
    best = max(seed_par, faithful)
    blas_name = (f"OpenBLAS 0.3.29 zgemm/zgesv ({os.path.basename(blas)}, 1 BLAS thread per call)" if blas
                 else "its own complex loops")
    alt = "; ".join(f"{'OpenBLAS' if k else 'loops'} {S / v:.3g} evals/s" for k, v in calib.items())
    blas_name += f" (faster backend in the calibration round: {alt})"
    return {
        "value": best,
        "unit": "evals/s",
        "cores": nthreads,
        "kind": "port",
        "sample": (f"oracle/cpu_ref.c (gcc -O3, OpenMP) with {blas_name} on {nthreads} threads of a {model} "
                   f"(nproc {ncpu}, affinity {aff}): {done} evals over the first {S2} of this rank's seeds, "
                   f"seed-parallel {seed_par:.3g} evals/s ({t2:.1f} s); reference-faithful k-parallel mode on 1 seed "
                   f"{faithful:.3g} evals/s; faster mode reported"),
    }, (J, g, S2)


SIDE_LEGS = "zz_batch:fused,tunable_bus:fused,cavity_dense:fused,cavity:split,zz_batch:split,tunable_bus:split"


def side_legs(spec, local_rank, order, steps, warmup, parity_seeds=4):
    """The other configs' rates in the same process (rank 0 at N = 1, after the contract line's timed region): per
    leg "config:form" a fresh engine on that config's rank-0 seeds, `warmup` untimed evals, `steps` timed ones
    (device sync on both sides), and parity of the first `parity_seeds` seeds against the C port (oracle/cpu_ref.c,
    checker only).  Not the metric: the contract's value is the main line's config."""
    import numpy as np
    import torch
    from qoc_amd import GrapeEngine, systems
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpuref  # checker only (oracle/)
    out = {}
    for leg in [s for s in spec.split(",") if s]:
        name, form = (leg.split(":") + ["fused"])[:2]
        t_leg = time.perf_counter()
        try:
            mk_prob, mk_u, B = systems.CONFIGS[name]
            prob = mk_prob()
            u_all = mk_u(B, 0)
            eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B, precision=prob.precision, device=local_rank)
            eng.set_cost_trace(prob.x_target, prob.n)
            dev = torch.device("cuda", local_rank)
            u_d = torch.from_numpy(np.ascontiguousarray(np.transpose(u_all, (0, 2, 1)))).to(dev)
            J_d = torch.empty(B, dtype=torch.float64, device=dev)
            g_d = torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device=dev)

            def step():
                if form == "split":
                    eng.propagate_device(u_d.data_ptr(), J_d.data_ptr())
                    eng.grape_sensitivity_device(u_d.data_ptr(), order, g_d.data_ptr())
                else:
                    eng.eval_device(u_d.data_ptr(), order, J_d.data_ptr(), g_d.data_ptr())

            for _ in range(warmup):
                step()
            eng.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            eng.synchronize()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            info = eng.info()
            S = min(parity_seeds, B)
            cpuref.use_blas(False)
            Jc, gc = cpuref.grape_eval_batch(prob, u_all[:S], order=order, mode=0, nthreads=cpu_threads())
            Jg = J_d[:S].cpu().numpy()
            gg = np.transpose(g_d[:S].cpu().numpy(), (0, 2, 1))
            eng.close()
            out[f"{name}:{form}"] = {
                "value": B * steps / el, "unit": "evals/s", "ms_per_step": el / steps * 1e3, "steps": steps,
                "warmup": warmup, "seeds": B, "workload": WORKLOADS[name],
                "path": {k: info.get(k) for k in ("path", "chain", "chain_kernel", "backward", "split_forward",
                                                  "interp_degree")},
                "parity_vs_cpu_port": {"seeds_checked": S, "max_abs_dJ": float(np.abs(Jg - Jc).max()),
                                       "max_rel_dJdu": float(max(np.linalg.norm(gg[b] - gc[b]) / np.linalg.norm(gc[b])
                                                                 for b in range(S)))},
                "leg_wall_s": time.perf_counter() - t_leg}
        except Exception as ex:  # a report beside the metric, never the metric
            out[f"{name}:{form}"] = {"value": None, "error": str(ex)}
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path, arrays, rank=0):
    """Write each array as <path>/<name>.npy (rank r > 0: <name>.rank<r>.npy), float32 arrays as they are and the
    rest as float64.  All of them together stay under DUMP_MAX_BYTES: an array above its even share of that is cut
    to a fixed sample of its flattened entries (seeded by the array's size, so the same entries in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_MAX_BYTES // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.asarray(a)
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(a.size).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + (f".rank{rank}" if rank else "") + ".npy"), a)


def launch_ranks(n: int) -> int:
    """Start n ranks of this script (torch.distributed.run, rendezvous on 127.0.0.1) and return their exit
    code.  Called before anything touches the GPU: the ranks are child processes, this one only waits."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def cpu_plumbing(args, rank: int, world: int) -> None:
    """The multi-rank plumbing without a GPU (gloo): every rank holds B synthetic objectives of its seed shard,
    the best (J, global seed) is exchanged K times with the barrier / max-over-ranks timing of the GPU run, and
    rank 0 prints the contract line (data "cpu-plumbing", no evals measured)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from qoc_amd import multi
    if world > 1:
        dist.init_process_group("gloo")
    B = args.seeds or 8
    J = torch.from_numpy(np.random.default_rng(rank).uniform(0.1, 1.0, B))
    for _ in range(args.warmup):
        best = multi.gather_best(J, rank * B)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        best = multi.gather_best(J, rank * B)
    if world > 1:
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "GRAPE gradient evals/sec (dim N, T slices, B seeds) @ 1/2/4/8 GPU", "value": None,
                          "unit": "evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": float(el.item()) / max(args.steps, 1) * 1e3, "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": None, "data": "cpu-plumbing",
                          "config": {"workload": "best-(J, seed) exchange only", "seeds_per_rank": B,
                                     "global_seeds": B * world, "parallelism": f"seed-sharded x{world}"},
                          "best_over_ranks": {"J": best[0], "seed": best[1], "transport": "torch.distributed (gloo)"}}),
              flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--warmup-ms", type=float, default=50.0,
                    help="after the W warmup steps, further untimed steps up to this much warm-up time (0: none)")
    ap.add_argument("--config", default="cavity", choices=sorted(WORKLOADS))
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=0, help="override seeds per GPU")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: leave the CPU baseline and its parity check out")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="with --full: CPU time of the baseline's sample")
    ap.add_argument("--call-form", default="fused", choices=["fused", "split", "ipopt"],
                    help="fused: qoc_eval_dev; split: qoc_propagate_dev + qoc_grape_sensitivity_dev; ipopt: the spline "
                         "callbacks qoc_propagate_spline + qoc_sensitivity_spline on host coefficients")
    ap.add_argument("--side", default=None,
                    help="with --full: comma list of config:form legs timed after the main line (rank 0, N = 1; default: "
                         "the other BASELINE configs when the main config is the default one, none otherwise; '' for "
                         "none)")
    ap.add_argument("--cpu-plumbing", action="store_true",
                    help="no GPU: check the launcher and the best-(J, seed) exchange over gloo (CPU tests)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the legs beside the metric: the CPU baseline with the parity "
                         "check against it (--no-cpu, --cpu-seconds) and the side legs (--side); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step returned (J, dJdu or dJdc, best) as "
                         "DIR/<name>.npy (ranks above 0: DIR/<name>.rank<r>.npy)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # one process per GPU: start the ranks (before anything touches the GPU) and report their exit code
        sys.exit(launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if args.cpu_plumbing:
        return cpu_plumbing(args, rank, world)

    import numpy as np
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)  # RCCL over xGMI

    from qoc_amd import GrapeEngine, systems

    mk_prob, mk_u, B_default = systems.CONFIGS[args.config]
    prob = mk_prob()
    B = args.seeds or B_default
    u_all = mk_u(B, rank)  # (B, nu, Nt), rank-seeded synthetic controls
    eng = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B, precision=prob.precision, device=local_rank)
    eng.set_cost_trace(prob.x_target, prob.n)
    coef = None
    if args.call_form == "ipopt":
        # Ipopt's variables: 10 cubic B-spline coefficients per control (examples/zz_coupling_ipopt_exp.jl:27-37), in
        # the config's control range; u = (Bs c)^T is what the kernels see (and what the parity leg checks)
        ns = 10
        Bs = systems.spline_matrix(float(prob.Nt), prob.Nt, ns)
        coef = np.random.default_rng(1000 + rank).uniform(u_all.min(), u_all.max(), size=(B, ns, prob.nu))
        u_all = np.ascontiguousarray(np.einsum("tn,bnj->bjt", Bs, coef))
        eng.set_spline_basis(Bs)

    # device-resident buffers in the engine's layout: u[b, k, j]
    u_d = torch.from_numpy(np.ascontiguousarray(np.transpose(u_all, (0, 2, 1)))).to(dev)
    J_d = torch.empty(B, dtype=torch.float64, device=dev)
    g_d = torch.empty(B, prob.Nt, prob.nu, dtype=torch.float64, device=dev)
    best_d = torch.empty(2, dtype=torch.float64, device=dev)
    gathered = torch.empty(2 * world, dtype=torch.float64, device=dev)
    stream = torch.cuda.ExternalStream(eng.stream(), device=dev)
    seed_offset = torch.arange(B, dtype=torch.float64, device=dev) + rank * B
    # the one exchange: best (J, global seed) over all ranks, RCCL inside libqoc_mi355x.so (qoc_allgather_best,
    # a real communicator also at world 1); torch.distributed's all_gather (also RCCL) only if the library
    # cannot load RCCL
    from qoc_amd import multi
    # RCCL prints its version banner on stdout when a communicator comes up: keep stdout for the one JSON line
    sys.stdout.flush()
    saved_fd = os.dup(1)
    os.dup2(2, 1)
    try:
        transport = multi.init_engine_comm(eng, rank * B)
    finally:
        sys.stdout.flush()
        os.dup2(saved_fd, 1)
        os.close(saved_fd)
    if world == 1:  # nothing to exchange: the evals that reduce their own J write the best pair here themselves
        eng.set_best_output(best_d.data_ptr())

    host_out = {}  # ipopt form: the host arrays the spline callbacks return

    def step():
        if args.call_form == "fused":
            eng.eval_device(u_d.data_ptr(), args.order, J_d.data_ptr(), g_d.data_ptr())
        elif args.call_form == "split":
            eng.propagate_device(u_d.data_ptr(), J_d.data_ptr())
            eng.grape_sensitivity_device(u_d.data_ptr(), args.order, g_d.data_ptr())
        else:
            host_out["J"] = eng.propagate_spline(coef)
            host_out["dJdc"] = eng.sensitivity_spline(coef, args.order)
        if transport in ("rccl-libqoc", "local"):
            eng.allgather_best_device(best_d.data_ptr())  # on the engine stream, after its kernels
        elif world > 1:
            with torch.cuda.stream(stream):  # ordered after the engine's kernels
                jm, idx = torch.min(J_d, 0)
                best_d[0] = jm
                best_d[1] = seed_offset[idx]
                dist.all_gather_into_tensor(gathered, best_d)

    for _ in range(args.warmup):
        step()
    eng.synchronize()
    torch.cuda.synchronize()
    # the W warmup steps leave a sub-millisecond step short of steady state (clocks, queues: cavity 0.094 ms per step
    # over the first 20 steps against 0.086 after 200, tools/step_fixed.py); so after them, further untimed steps
    # until --warmup-ms of warm-up (the same count on every rank: each step has a collective), reported as
    # warmup_steps_run
    extra = 0
    if args.warmup > 0 and args.warmup_ms > 0:
        tw = time.perf_counter()
        while extra < 2000:
            go = (time.perf_counter() - tw) * 1e3 < args.warmup_ms
            if world > 1:  # rank 0 decides, so every rank runs the same steps
                f = torch.tensor([1 if go else 0], dtype=torch.int32, device=dev)
                dist.broadcast(f, src=0)
                go = bool(f.item())
            if not go:
                break
            n = max(1, min(10, 2000 - extra))
            for _ in range(n):
                step()
            extra += n
            eng.synchronize()
        torch.cuda.synchronize()

    eng.pade_histogram(reset=True)
    eng.taylor_histogram(reset=True)
    eng.chain_terms(reset=True)
    eng.phase_times(reset=True)
    info0 = eng.info()
    if info0["path"] == "large_n":
        eng.gemm_stats(reset=True)
    eng.set_profiling(True)
    if world > 1:
        dist.barrier()
    eng.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    eng.synchronize()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    eng.set_profiling(False)
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())

    if args.dump_outputs:
        # what a caller of the timed path holds after the last step: the device arrays J (B,), dJdu (B, Nt, nu) of the
        # device call forms, the spline callbacks' J (B,), dJdc (B, ns, nu) of the ipopt form, and the best (J, seed)
        outs = dict(host_out) if args.call_form == "ipopt" else {"J": J_d.cpu().numpy(), "dJdu": g_d.cpu().numpy()}
        outs["best"] = best_d.cpu().numpy()
        dump_outputs(args.dump_outputs, outs, rank)

    phases = eng.phase_times()
    if args.call_form == "ipopt" and args.full:  # the parity leg checks the split kernels on the spline controls' u
        eng.propagate_device(u_d.data_ptr(), J_d.data_ptr())
        eng.grape_sensitivity_device(u_d.data_ptr(), args.order, g_d.data_ptr())
        eng.synchronize()
    hist = eng.pade_histogram()
    thist = eng.taylor_histogram()
    terms = eng.chain_terms()  # Taylor-action chains: Σ P s over all slices, per direction
    K = args.steps
    N, m, nu, Nt = prob.N, prob.m, prob.nu, prob.Nt
    esz = 16 if prob.precision == "fp64" else 8
    value = B * world * K / elapsed

    # ---- roofline of each kernel, dominant one reported ----
    per_launch = {k: (ms / n if n else 0.0) for k, (ms, n) in phases.items()}
    # launches per step: the overlapped backward runs the chain and the gradient in slice ranges (several
    # launches per step); per-launch work = per-step work / launches per step.  A kernel that never launched
    # reports 0 launches and 0 ms
    lps = {k: n / K for k, (ms, n) in phases.items()}
    per_step = {k: ms / K for k, (ms, n) in phases.items()}
    hist_launch = {k: v / K for k, v in hist.items()}
    peak = PEAK_TFLOPS[prob.precision]
    info1 = eng.info()
    large = info1["path"] == "large_n"
    traffic_file = os.path.join(ROOT, "profiles", f"traffic_{args.config}.json")
    if args.call_form != "fused":  # the split forms run other kernels (tools/profile.sh <config> <tag> <form>)
        alt = os.path.join(ROOT, "profiles", f"traffic_{args.config}_{args.call_form}.json")
        traffic_file = alt if os.path.exists(alt) else traffic_file
    traffic_all, traffic_src = {}, None
    if os.path.exists(traffic_file):
        try:
            tj = json.load(open(traffic_file))
            # {"source": profile summary, "run": run id, "kernels": {kernel: HBM bytes per launch}} (older files:
            # the kernel map alone)
            traffic_all = tj.get("kernels", tj) if isinstance(tj, dict) else {}
            traffic_src = {"file": os.path.relpath(traffic_file, ROOT), "source": tj.get("source"),
                           "run": tj.get("run"), "counters": tj.get("counters")}
        except Exception:
            traffic_all = {}
    taylor = info1.get("chain") == "taylor" and not large
    seg = info1.get("backward") == "segmented"  # the one-launch segmented block eval (k_blkseg_eval)
    # blocks of 5..16 rows on stored propagators (k_blkp_exp + k_blkp_dual + k_blkp_grad, csrc/qoc_blkp.hpp)
    p16 = info1.get("chain_kernel") == "blocks_prop16"
    dual = info1.get("concurrent_launch") == "dual"
    fused = info1.get("concurrent_launch") == "fused"  # block propagators: forward, then the backward with the gradient
    bsz = block_sizes(prob) if taylor and info1.get("chain_kernel") in ("blocks", "blocks_mfma", "blocks_prop") else None
    bprop = info1.get("chain_kernel") == "blocks_prop"
    # blocks of <= 4 rows (VALU lanes or packed MFMA block waves) with the block gradient; 5..16 rows: MFMA block
    # waves with the dense gradient
    blocks = bsz is not None and bsz.max() <= 4 and not seg
    rot_blocks = bsz is not None and bsz.max() > 4
    if seg:
        # one launch per eval: segment products, prefix scan, every segment backwards with the gradient (phase slot
        # k_chain_bwd); HBM traffic is u in (and its two copies out), J / λ_N coefficients and dJdu out -- x_k, λ_k and
        # U_k stay on chip, so the kernel is bound by its fp64 VALU work (executed flops, blkseg_unit_flops)
        bsz_s = block_sizes(prob)
        nbk = int(bsz_s.max())
        nblk = len(bsz_s)
        p_avg = terms / K / max(B * Nt, 1)  # Taylor degree (blocks of 3 rows; the kernel counts Nt P 2^J per seed)
        units = B * Nt * nblk
        if nbk == 2:  # the series degree per seed
            ks = blkseg_series_k(prob, u_all)
            # the controls' blocks without diagonal (and so without shifts): the kernel's ZD path
            zd = all(not np.any(np.diag(np.asarray(a))) for a in prob.A)
            fl = [blkseg_unit_flops(2, args.order, None, int(k), zd) for k in ks]
            f1, f3 = float(np.mean([a for a, _ in fl])), float(np.mean([c for _, c in fl]))
        else:
            ks = None
            f1, f3 = blkseg_unit_flops(nbk, args.order, p_avg)
        sdeg = {str(int(k)): int(np.sum(ks == k)) for k in np.unique(ks)} if ks is not None else None
        # the split call form: the forward launch (phases 0-2, phase slot k_chain_fwd) writes G at the S segment ends
        # (B S nblk nb^2 complex), the backward launch (phase 3, slot k_chain_bwd) reads them back
        split_seg = lps["k_chain_fwd"] > 0
        gbytes = B * blkseg_segments(B, Nt, nblk) * nblk * nbk * nbk * 16
        parts = ([("k_blkseg_fwd", "k_chain_fwd", f1, B * Nt * nu * 8 * 2 + B * (8 + 2 * m * 16) + gbytes),
                  ("k_blkseg_bwd", "k_chain_bwd", f3, B * Nt * nu * 8 * 3 + B * 2 * m * 16 * 2 + gbytes)]
                 if split_seg else
                 [("k_blkseg_eval", "k_chain_bwd", f1 + f3, B * Nt * nu * 8 * 4 + B * (8 + 2 * 2 * m * 16))])
        kern = {}
        for kname, slot, fu, hbm in parts:
            flops = units * fu
            t = per_step[slot] / 1e3
            ach = flops / 1e12 / t if t > 0 else 0.0
            kern[kname] = {
                "ms_per_launch": per_launch[slot], "launches_per_step": lps[slot], "bound": "valu",
                "achieved": ach, "unit": "TFLOP/s", "peak": peak, "frac": ach / peak,
                "executed_gflop_per_launch": flops / 1e9,
                "flops_per_unit": {"phase1": f1, "phase3": f3} if not split_seg else fu,
                "units_per_launch": units, "hbm_bytes_per_launch": hbm,
                "hbm_gbs": hbm / 1e9 / t if t > 0 else 0.0, "taylor_degree": p_avg if nbk == 3 else None,
                "series_degree_k": sdeg}
        for k in ("k_expm", "k_grad"):
            kern[k] = {"ms_per_launch": per_launch[k], "launches_per_step": lps[k]}
        dom_k, dom_slot = max(((kn, sl) for kn, sl, _, _ in parts), key=lambda x: per_step[x[1]])
        ach = kern[dom_k]["achieved"]
        roof = {"kernel": dom_k, "bound": "valu", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                "frac": ach / peak, "traffic": traffic_all.get(dom_k), "traffic_source": traffic_src,
                "ms_per_launch": per_launch[dom_slot], "launches_per_step": lps[dom_slot],
                "blocks": [int(x) for x in bsz_s],
                "note": ("segmented block eval, one launch per eval (csrc/qoc_blkseg.hpp): achieved = executed fp64 "
                         "flops per launch (bench.py blkseg_unit_flops x B Nt nblk) / launch time, against the fp64 "
                         "peak (vector = dense MFMA, 78.6 TF/s); HBM traffic is u, J and dJdu only "
                         "(hbm_bytes_per_launch), so the bound is the VALU issue, not bandwidth")}
    elif p16:
        # stored propagators: per (seed, slice, live block) one 16 x 16 exponential on v_mfma_f64_16x16x4 (executed
        # products counted by the kernel: qoc_chain_terms; 12 MFMAs of 2048 flops each, the three-real-product form),
        # the two one-matvec chains each reading the one stored propagator (4 KB per slice and direction) and writing
        # the live rows' states,
        # and the batched gradient (per 16 slices: 2(nu+1) co-state and 3 nu + 2 state-side 16 x 16 x 16 complex GEMMs
        # per live block and column, 12 MFMAs each)
        lsz = live_block_sizes(prob)
        nlive = len(lsz)
        prods = terms / K  # executed 16 x 16 complex products per step
        f_exp = prods * 12 * 2048.0
        tiles = B * -(-Nt // 16)
        f_grad = tiles * nlive * m * (2 * (nu + 1) + 3 * nu + 2) * 12 * 2048.0
        u_bytes = B * Nt * nlive * 256 * 16  # written once by the formation
        one_chain = u_bytes + B * Nt * float(np.sum(lsz)) * m * 16  # one direction: read every U_k, write the states
        # the split call form runs the two directions as separate launches (k_blkp_chain: forward in propagate, μ in
        # grape_sensitivity); the eval runs both in one (k_blkp_dual)
        split16 = lps["k_chain_bwd"] > 0
        # one control: the propagators interpolated in u (k_blkp_int: Σ_{i<=D} T_i(ξ) M_i, 4 flops per complex entry
        # and term, no MFMA); its algorithmic traffic is the 4 KB propagator written per unit
        ideg = info1.get("interp_degree", 0)
        f_int = B * Nt * nlive * 256 * (ideg + 1) * 4.0
        # the interpolating chains (k_blkp_ichain, info interp_chain 1 / 2): each chain wave forms its slices'
        # propagators in registers (every entry, or the 128 packed upper-triangle slots of symmetric propagators), once
        # per direction, then the one-matvec step; HBM: u and the slices' phases read, the live rows' states written
        ichain = int(info1.get("interp_chain", 0))
        ient = 256 if ichain == 1 else 128
        dirs_i = 1 if split16 else 2
        f_ichain = dirs_i * B * Nt * nlive * (ient * (ideg + 1) * 4.0 + 8.0 * 256 * m)
        b_ichain = dirs_i * (B * Nt * (8 + 16) + B * Nt * float(np.sum(lsz)) * m * 16)
        models = {
            "k_expm": ("hbm", u_bytes / 1e9, "GB/s", PEAK_HBM_GBS) if ideg else ("mfma", f_exp / 1e12, "TFLOP/s", peak),
            "k_chain_fwd": ("hbm", (1 if split16 else 2) * one_chain / 1e9, "GB/s", PEAK_HBM_GBS),
            "k_chain_bwd": ("hbm", one_chain / 1e9 if split16 else 0.0, "GB/s", PEAK_HBM_GBS),
            "k_grad": ("mfma", f_grad / 1e12, "TFLOP/s", peak),
        }
        if ichain:
            models["k_chain_fwd"] = ("valu", f_ichain / 1e12, "TFLOP/s", peak)
            models["k_chain_bwd"] = ("valu", f_ichain / 1e12 if split16 else 0.0, "TFLOP/s", peak)
    elif blocks:
        # block chains (csrc/qoc_blk.hpp, qoc_blku.hpp); the launch's algorithmic bytes are the states it writes (x_k,
        # and μ_k in the dual launch) plus what it reads per slice: the step records of k_tchain_prep (32 B record +
        # P+1 Chebyshev coefficients + u_k) for the polynomial-in-the-chain kernels, u_k alone for the block
        # propagators (their step records are formed in the kernel); the gradient reads x_k and λ_{k+1} once and
        # writes dJdu
        nb2 = float(np.sum(block_sizes(prob).astype(np.float64) ** 2))
        dirs = 2 if dual else 1
        tl = terms / K * dirs
        p_avg = terms / K / max(B * Nt, 1)
        # block propagators: k_blku_rec reads u_k and writes one 64-byte step record per slice (Nt rounded up to
        # 64), which the chains read back; the fused backward (k_blku_bwdg) reads x_0..x_{Nt-1} and the records and
        # writes dJdu -- λ never leaves the workgroup and no gradient launch follows
        ntp = -(-Nt // 64) * 64
        rec = B * Nt * 64 if bprop else B * Nt * (32 + 8 * (p_avg + 1) + 8 * nu)
        st = B * (Nt + 1) * N * m * esz
        bwd_bytes = (st + rec) if not fused else (B * Nt * N * m * esz + rec + B * Nt * nu * 8)
        models = {
            "k_expm": ("hbm", (B * Nt * 8 * nu + B * ntp * 64 if bprop
                               else B * Nt * (8 * nu + 32 + 8 * (p_avg + 1))) / 1e9, "GB/s", PEAK_HBM_GBS),
            "k_chain_fwd": ("hbm", dirs * (st + rec) / 1e9, "GB/s", PEAK_HBM_GBS),
            "k_chain_bwd": ("hbm", bwd_bytes / 1e9, "GB/s", PEAK_HBM_GBS),
            "k_grad": ("hbm", (2 * B * Nt * N * m * esz + 16 * nu * B * Nt) / 1e9, "GB/s", PEAK_HBM_GBS),
        }
        if bprop:
            # executed fp64 VALU work: per (slice, block) the propagator's Taylor terms in the Cayley-Hamilton basis
            # (n_b complex multiply-adds per term) plus forming A_k and U_k (~130 flops at n_b = 2), per slice one
            # n_b x n_b complex matvec per column; the gradient: K (m n_b^2 CMAC), 2(o-1) products of n_b x n_b
            # blocks and nu traces (8 flops per CMAC)
            nbk = block_sizes(prob).astype(np.float64)
            form = float(np.sum(8.0 * nbk * p_avg + 16.0 * nbk ** 3 + 40.0 * nbk ** 2)) * B * Nt
            gflops = 8.0 * B * Nt * float(np.sum(m * nbk ** 2 + 2 * (args.order - 1) * nbk ** 3 + nu * nbk ** 2))
            block_flops = {"k_chain_fwd": dirs * (form + 8.0 * nb2 * m * B * Nt),
                           "k_chain_bwd": form + 8.0 * nb2 * m * B * Nt + (gflops if fused else 0.0),
                           "k_grad": 0.0 if fused else gflops}
        else:
            block_flops = {"k_chain_fwd": 8.0 * nb2 * m * tl, "k_chain_bwd": 8.0 * nb2 * m * terms / K,
                           "k_grad": 8.0 * nb2 * m * B * Nt * (2 * (args.order - 1) + nu * args.order)}
    elif taylor:
        # Taylor-action chains (csrc/qoc_tchain.hpp): no exponential kernel; the chains carry the Taylor terms,
        # each an N x N by N x m complex matvec (8 N^2 m flops) on v_mfma_f64_4x4x4 (fp64) / VALU (fp32); the dual
        # launch (k_tchain_mf_dual) carries both directions' terms.  MFMA block waves (k_blkrot_*, qoc_blk.hpp):
        # per term 8 v_mfma_f64_4x4x4_4b (4 x 128 flops each) per (block, column pair) wave
        tl = terms / K * (2 if dual else 1)
        mv_flops = 8.0 * N * N * m
        if rot_blocks:
            # algorithmic block work: one n_b x n_b complex matvec per block and column (8 n_b^2 m flops), not the
            # executed MFMA flops of the 16-row padded waves (8 v_mfma_f64_4x4x4_4b of 4 x 128 flops per column pair)
            dead_skip = dual and os.environ.get("QOC_BLK_DEAD", "1") != "0"
            mv_flops = 8.0 * float(np.sum((live_block_sizes(prob) if dead_skip else block_sizes(prob))
                                          .astype(np.float64) ** 2)) * m
        models = {
            "k_expm": ("mfma", 0.0, "TFLOP/s", peak),  # k_tchain_prep: (P, s, e^mu) per slice, no flops counted
            "k_grad": ("mfma", grad_flops(N, m, nu, Nt, B, args.order,
                                          info1.get("backward") in ("captured", "concurrent", "blocks")) / 1e12,
                       "TFLOP/s", peak),
            "k_chain_fwd": ("mfma", mv_flops * tl / 1e12, "TFLOP/s", peak),
            "k_chain_bwd": ("mfma", mv_flops * tl / 1e12, "TFLOP/s", peak),
        }
    elif not large:
        models = {
            "k_expm": ("mfma", (taylor_flops(N, {k: v / K for k, v in thist.items()}) if thist
                                else expm_flops(N, hist_launch)) / 1e12, "TFLOP/s", peak),
            "k_grad": ("mfma", grad_flops(N, m, nu, Nt, B, args.order) / 1e12, "TFLOP/s", peak),
            "k_chain_fwd": ("hbm", chain_bytes(N, m, Nt, B, esz) / 1e9, "GB/s", PEAK_HBM_GBS),
            "k_chain_bwd": ("hbm", (chain_bytes(N, m, Nt, B, esz) + B * (Nt + 1) * N * m * esz) / 1e9, "GB/s",
                            PEAK_HBM_GBS),
        }
    else:
        # phases of the chunked GEMM pipeline (each a sequence of launches); executed GEMM FLOPs
        nchunks = math.ceil(B * Nt / info1["chunk"])
        ns_it = (info1["ns_iters"] - info0["ns_iters"]) / max(nchunks * K, 1)
        if thist:
            f_expm = taylor_flops(N, {k: v / K for k, v in thist.items()}, large=True)
        else:
            g_expm = sum(c * (GEMMS_PER_DEGREE[d] + s) for (d, s), c in hist_launch.items())
            slices = sum(hist_launch.values())
            f_expm = 8.0 * N ** 3 * (g_expm + slices * (2 * ns_it + 1))
        f_chain = 8.0 * N * N * m * B * Nt
        # order 3 with m > 2N/3 (synthetic: m = N): five products of G = λ x^H (one N^2 m, four N^3; big_backward),
        # else 2(o-1) + o N^2 m-GEMM equivalents (P_a, Q_b, M' = W P^H)
        sandwich = args.order == 3 and 4 * N < 6 * m
        if os.environ.get("QOC_GRAD_SANDWICH") is not None:
            sandwich = args.order == 3 and int(os.environ["QOC_GRAD_SANDWICH"]) != 0
        if sandwich:
            f_grad = 8.0 * B * Nt * (N * N * m + 4.0 * N ** 3)
        else:
            f_grad = 8.0 * N * N * m * B * Nt * (2 * (args.order - 1) + args.order)
        models = {
            "k_expm": ("mfma", f_expm / 1e12, "TFLOP/s", peak),
            "k_chain_fwd": ("mfma", f_chain / 1e12, "TFLOP/s", peak),
            "k_chain_bwd": ("mfma", f_chain / 1e12, "TFLOP/s", peak),
            "k_grad": ("mfma", f_grad / 1e12, "TFLOP/s", peak),
        }
    if seg:
        models = {}
    else:
        kern = {}
    for k, (bound, work, unit, pk) in models.items():
        t = per_step[k] / 1e3
        ach = work / t if t > 0 else 0.0
        kern[k] = {"ms_per_launch": per_launch[k], "launches_per_step": lps[k], "bound": bound, "achieved": ach,
                   "unit": unit, "peak": pk, "frac": ach / pk}
    names = {"k_expm": "k_expm_rr", "k_chain_fwd": "k_chain_fwd", "k_chain_bwd": "k_chain_bwd", "k_grad": "k_grad_rr"}
    if seg:
        pass  # kern and roof set above
    elif p16:
        names = {"k_expm": "k_blkp_int" if ideg else "k_blkp_exp",
                 "k_chain_fwd": "k_blkp_chain" if split16 else "k_blkp_dual",
                 "k_chain_bwd": "k_blkp_chain" if split16 else "k_blkp_dual", "k_grad": "k_blkp_grad"}
        if ichain:
            names.update({"k_chain_fwd": "k_blkp_ichain", "k_chain_bwd": "k_blkp_ichain"})
        live_k = ("k_expm", "k_chain_fwd", "k_chain_bwd", "k_grad") if split16 else ("k_expm", "k_chain_fwd", "k_grad")
        if ichain:
            live_k = tuple(k for k in live_k if k != "k_expm")
        for k in live_k:
            kern[k]["kernel"] = names[k]
        # per-launch figures: the step's work over its launches (the formation runs once per seed group)
        if ichain:
            kern["k_expm"] = {"ms_per_launch": 0.0, "launches_per_step": 0.0, "interp_degree": ideg,
                              "note": "no formation launch: the chains interpolate their propagators (k_blkp_ichain)"}
        else:
            kern["k_expm"]["products_per_unit"] = prods / max(B * Nt * nlive, 1)
            kern["k_expm"]["executed_gflop_per_launch"] = (f_int if ideg else f_exp) / 1e9 / max(lps["k_expm"], 1.0)
            if ideg:
                kern["k_expm"]["interp_degree"] = ideg
                t = per_step["k_expm"] / 1e3
                kern["k_expm"]["executed_tflops"] = f_int / 1e12 / t if t > 0 else 0.0
            kern["k_expm"]["hbm_bytes_per_launch"] = u_bytes / max(lps["k_expm"], 1.0)
        for k in ("k_chain_fwd", "k_chain_bwd") if split16 else ("k_chain_fwd",):
            kern[k]["hbm_bytes_per_launch"] = (b_ichain if ichain else models[k][1] * 1e9) / max(lps[k], 1.0)
            kern[k]["ns_per_serial_step"] = per_launch[k] * 1e6 / Nt
            if ichain:
                kern[k]["executed_gflop_per_launch"] = f_ichain / 1e9 / max(lps[k], 1.0)
        kern["k_chain_fwd"]["note"] = (("interpolating chains (k_blkp_ichain): each (seed, direction) wave forms its "
                                        "slices' propagators from the interpolation coefficients in LDS ("
                                        + ("the symmetric propagators' upper triangle" if ichain == 2 else "every entry")
                                        + "), then one matvec per slice; achieved = executed fp64 flops of both / time "
                                        "(the step is latency- and issue-bound at one wave per SIMD)") if ichain else
                                       ("forward chain alone (propagate), one matvec per slice from the stored "
                                        "propagators (LDS-DMA staged); k_chain_bwd: the mu recurrence alone "
                                        "(grape_sensitivity)") if split16 else
                                       ("forward chain and mu recurrence of every seed in one launch, one matvec per "
                                        "slice from the stored propagators (LDS-DMA staged)"))
        kern["k_grad"]["executed_gflop_per_launch"] = f_grad / 1e9 / max(lps["k_grad"], 1.0)
        dom = max(live_k, key=lambda k: per_step[k])
        roof = {"kernel": names[dom], "bound": kern[dom]["bound"], "achieved": kern[dom]["achieved"],
                "peak": kern[dom]["peak"], "unit": kern[dom]["unit"], "frac": kern[dom]["frac"],
                "traffic": traffic_all.get(names[dom]), "traffic_source": traffic_src,
                "ms_per_launch": kern[dom]["ms_per_launch"], "launches_per_step": lps[dom],
                "blocks": [int(x) for x in block_sizes(prob)], "live_blocks": [int(x) for x in lsz],
                "interp_chain": ichain,
                "note": kern["k_chain_fwd"]["note"] if ichain else
                        ("stored block propagators (csrc/qoc_blkp.hpp): the dominant kernel forms every slice's "
                         "16 x 16 block exponential on MFMA (Taylor / Paterson-Stockmeyer + squarings, degree and "
                         "squarings per slice); achieved = executed MFMA flops (12 v_mfma_f64_16x16x4 of 2048 "
                         "flops per complex product, products counted by the kernel) / launch time, against the "
                         "dense fp64 MFMA peak")}
    elif blocks:
        kb = {"blocks_mfma": "k_blkrot", "blocks_prop": "k_blku"}.get(info1.get("chain_kernel"), "k_blk")
        names = {"k_expm": "k_blku_rec" if bprop else "k_tchain_prep", "k_chain_fwd": kb + ("_dual" if dual else "_fwd"),
                 "k_chain_bwd": kb + ("_bwdg" if fused else "_bwd"), "k_grad": "k_blku_grad" if bprop else "k_blk_grad"}
        for k in ("k_chain_fwd", "k_chain_bwd", "k_grad"):
            kern[k]["kernel"] = names[k]
            t = per_step[k] / 1e3
            kern[k]["executed_tflops"] = block_flops[k] / 1e12 / t if t > 0 else 0.0
        for k in ("k_chain_fwd", "k_chain_bwd"):
            if not lps[k]:
                continue
            kern[k]["terms_per_seed"] = terms / K / B
            if bprop:
                # serial steps: Nt block matvecs per seed and direction (the propagators are formed beside them);
                # model: the n_b x n_b complex matvec, 4 n_b^2 dependent-free fp64 FMAs issued at 4 cycles each +
                # n_b 16-byte stores, at 2.1 GHz
                nbm = int(block_sizes(prob).max())
                kern[k]["serial_steps_per_seed"] = Nt
                kern[k]["ns_per_serial_step"] = per_launch[k] * 1e6 / Nt
                kern[k]["serial_step_model_ns"] = (16.0 * nbm * nbm + 8.0 * nbm) / 2.1
            else:
                kern[k]["ns_per_serial_term"] = per_launch[k] * 1e6 / max(terms / K / B, 1e-9)
        dom = max(("k_expm", "k_chain_fwd", "k_chain_bwd", "k_grad"), key=lambda k: per_step[k])
        roof = {"kernel": names[dom], "bound": kern[dom]["bound"], "achieved": kern[dom]["achieved"],
                "peak": kern[dom]["peak"], "unit": kern[dom]["unit"], "frac": kern[dom]["frac"],
                "traffic": traffic_all.get(names[dom]), "traffic_source": traffic_src,
                "ms_per_launch": kern[dom]["ms_per_launch"], "launches_per_step": lps[dom],
                "blocks": [int(x) for x in block_sizes(prob)],
                "note": ("block chains (generators with invariant blocks): achieved = algorithmic HBM bytes per launch "
                         "(states written, step records / u_k read; the gradient: x_k and λ_{k+1} read) / launch time"
                         + ("; the forward chain and the μ recurrence of every seed in one launch (" +
                            names["k_chain_fwd"] + ")" if dual else "")
                         + ("; the backward chain contracts the gradient beside it (" + names["k_chain_bwd"] +
                            "): x_k read once, λ kept in LDS" if fused else ""))}
    elif taylor:
        mf = prob.precision == "fp64"
        names = {"k_expm": "k_tchain_prep",
                 "k_chain_fwd": "k_tchain_mf_dual" if dual else "k_tchain_mf_fwd" if mf else "k_tchain_fwd",
                 "k_chain_bwd": "k_tchain_mf_bwd" if mf else "k_tchain_bwd",
                 "k_grad": "k_grad_rr_c" if info1.get("backward") in ("captured", "concurrent", "blocks") else "k_grad_rr"}
        if rot_blocks:
            names.update({"k_chain_fwd": "k_blkrot_dual" if dual else "k_blkrot_fwd", "k_chain_bwd": "k_blkrot_bwd"})
        for k in ("k_chain_fwd", "k_chain_bwd"):
            # serial Taylor terms of one seed per launch and the time each takes (the chains' critical path)
            kern[k]["kernel"] = names[k]
            kern[k]["terms_per_seed"] = terms / K / B  # per direction
            kern[k]["ns_per_serial_term"] = per_launch[k] * 1e6 / max(terms / K / B, 1e-9)
        dom = max(("k_chain_fwd", "k_chain_bwd", "k_grad"), key=lambda k: per_step[k])
        if dual:
            kern["k_chain_fwd"]["note"] = names["k_chain_fwd"] + ": forward chain and mu recurrence of every seed in one launch"
        roof = {"kernel": names[dom], "bound": kern[dom]["bound"], "achieved": kern[dom]["achieved"],
                "peak": kern[dom]["peak"], "unit": kern[dom]["unit"], "frac": kern[dom]["frac"],
                "traffic": traffic_all.get(names[dom]), "traffic_source": traffic_src,
                "ms_per_launch": kern[dom]["ms_per_launch"], "launches_per_step": lps[dom],
                "note": ("latency-bound serial recurrence (one workgroup per seed, Taylor terms in sequence): "
                         "achieved = executed matvec flops / launch time"
                         + ("; the backward (μ) recurrence runs beside the forward chain (" + names["k_chain_fwd"] +
                            ": one launch of 2B workgroups; flops of both directions), the contraction after both"
                            if dual else "; the backward (μ) recurrence runs beside the forward chain on a second "
                            "stream, the contraction after both" if info1.get("backward") == "concurrent" else "")
                         + ("; the backward chain runs in slice ranges, each range's gradient overlapped with "
                            "the next range" if lps.get("k_chain_bwd", 1) > 1 else ""))}
    elif not large:
        dom = max(per_step, key=per_step.get)
        # the exponential phase runs the register-resident kernels (k_expm_rr: T12 / Paterson-Stockmeyer)
        # unless QOC_EXPM_LDS or QOC_EXPM_PADE selects the LDS kernel k_expm
        lds_expm = info1.get("expm") != "taylor_rr"  # the reference's Padé or the LDS Paterson-Stockmeyer: k_expm
        kname = dom
        if dom == "k_expm" and not lds_expm:
            # one-pass k_expm_rr_mix when ||A_0||_1 > 4 theta_12 (tunable bus), else k_expm_rr (+ its
            # Paterson-Stockmeyer pass); the committed PMC summary names the one that ran
            kname = "k_expm_rr_mix" if "k_expm_rr_mix" in traffic_all and "k_expm_rr" not in traffic_all else "k_expm_rr"
        roof = {"kernel": kname, "bound": kern[dom]["bound"], "achieved": kern[dom]["achieved"],
                "peak": kern[dom]["peak"], "unit": kern[dom]["unit"], "frac": kern[dom]["frac"],
                "traffic": traffic_all.get(kname, traffic_all.get(dom)), "traffic_source": traffic_src,
                "ms_per_launch": kern[dom]["ms_per_launch"]}
    else:
        # dominant kernel = the batched complex GEMM (every phase is mostly k_bgemm launches)
        gs = eng.gemm_stats()
        ach = gs["flops"] / 1e12 / (gs["ms"] / 1e3) if gs["ms"] > 0 else 0.0
        kern["phases_note"] = "large-N path: k_expm/k_chain_*/k_grad entries are phase totals per step"
        roof = {"kernel": "k_bgemm", "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                "frac": ach / peak, "traffic": traffic_all.get("k_bgemm_glds", traffic_all.get("k_bgemm")),
                "traffic_source": traffic_src,
                "ms_per_launch": gs["ms"] / max(gs["launches"], 1),
                "launches_per_step": gs["launches"] / K,
                "gflop_per_launch": gs["flops"] / max(gs["launches"], 1) / 1e9,
                "ns_iters_per_chunk": ns_it, "chunk": info1["chunk"]}
    ref_f = ref_eval_flops(N, m, nu, {k: v / B for k, v in hist_launch.items()}, args.order)

    best = best_d.cpu().numpy().tolist()
    cpu = None
    parity = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        nthreads = cpu_threads()
        try:
            if large:
                cpu, (Jc, gc, n2) = cpu_baseline_large(prob, u_all, args.order, nthreads, args.cpu_seconds)
                # parity on the same truncated problem: seed 0, first n2 slices, through the GPU engine
                e2 = GrapeEngine(prob.A0, prob.A, prob.x0, n2, B=1, precision=prob.precision, device=local_rank)
                e2.set_cost_trace(prob.x_target, prob.n)
                u2 = np.ascontiguousarray(u_all[:1, :, :n2])
                Jg = e2.propagate(u2)
                gg = e2.grape_sensitivity(u2, args.order)
                e2.close()
                parity = {"seeds_checked": 1, "slices": int(n2), "max_abs_dJ": float(abs(Jg[0] - Jc)),
                          "max_rel_dJdu": float(np.linalg.norm(gg[0] - gc) / np.linalg.norm(gc))}
            else:
                cpu, (Jc, gc, S) = cpu_baseline(prob, u_all, args.order, nthreads, args.cpu_seconds)
                Jg = J_d[:S].cpu().numpy()
                gg = np.transpose(g_d[:S].cpu().numpy(), (0, 2, 1))
                parity = {"seeds_checked": int(S), "max_abs_dJ": float(np.abs(Jg - Jc).max()),
                          "max_rel_dJdu": float(max(np.linalg.norm(gg[b] - gc[b]) / np.linalg.norm(gc[b])
                                                    for b in range(S)))}
        except Exception as ex:  # the baseline is a report, not the product
            cpu = {"value": None, "unit": "evals/s", "cores": nthreads, "kind": "port", "sample": f"failed: {ex}"}

    side = None
    comm_ranks = eng.comm_ranks()
    spec = args.side if args.side is not None else (SIDE_LEGS if args.config == "cavity" and args.call_form == "fused"
                                                    and not args.seeds else "")
    if rank == 0 and world == 1 and args.full and spec:
        eng.close()
        eng = None
        side = side_legs(spec, local_rank, args.order, max(args.steps, 5), max(args.warmup, 2))

    if rank == 0:
        out = {
            "metric": "GRAPE gradient evals/sec (dim N, T slices, B seeds) @ 1/2/4/8 GPU",
            "value": value,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": K,
            "warmup": args.warmup,
            "warmup_steps_run": args.warmup + extra,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64" if prob.precision == "fp64" else "f32",
            "data": "synthetic",
            "config": {"workload": WORKLOADS[args.config], "name": args.config, "N": N, "m": m, "nu": nu,
                       "Nt": Nt, "seeds_per_gpu": B, "global_seeds": B * world, "order": args.order,
                       "call_form": args.call_form,
                       "parallelism": f"seed-sharded x{world}"},
            "roofline": roof,
            "cpu_baseline": cpu,
            "kernels": kern,
            "pade_hist_per_step": {f"d{d}s{s}": v / K for (d, s), v in sorted(hist.items())},
            "taylor_hist_per_step": {f"m{mm}s{s}": v / K for (mm, s), v in sorted(thist.items(), key=str)},
            # the reference algorithm's flops per eval (SURVEY §8d F_eval, Padé (d, s) counted on the device)
            # times this engine's eval rate: a reference-equivalent RATE, not a utilisation figure (the engine
            # executes far fewer flops than that formula; see "roofline" for the executed work)
            "reference_equivalent": {"gflop_per_eval": ref_f / 1e9, "rate_tflops": ref_f * value / 1e12,
                                     "note": "reference-algorithm flops x eval rate; not executed work, may exceed peak"},
            "parity_vs_cpu_port": parity,
            "engine": info1,
            "best_over_ranks": {"J": best[0], "seed": int(best[1]), "transport": transport,
                                "communicator_ranks": comm_ranks},
        }
        if cpu and cpu.get("value"):
            out["speedup_vs_cpu"] = value / cpu["value"]
        if side is not None:
            out["side_legs"] = side
        print(json.dumps(out), flush=True)
    if eng is not None:
        eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
