"""Shared recipes of the segmented block eval's GPU tests (tests/test_gpu_blkseg*.py): the engine with its
environment switches, the device call forms, the fp64 bar of SURVEY.md §8c per seed (|ΔJ| <= 1e-12,
||ΔdJdu|| / ||dJdu|| <= 1e-10), the shipped cases with their penalties and the random permuted block problem.
"""
import functools

import numpy as np

MU = 0.37


def engine(prob, B, monkeypatch, pen=None, seg="1", S=None, W=None, segpen=None, segex=None):
    """A GrapeEngine on the block path with the trace cost; every QOC_BLKSEG_* switch is set or cleared here."""
    from qoc_amd import GrapeEngine
    monkeypatch.setenv("QOC_BLOCKS", "1")
    monkeypatch.setenv("QOC_BLKU", "1")
    monkeypatch.setenv("QOC_BLKSEG", seg)
    monkeypatch.delenv("QOC_BLKSEG_SPLIT", raising=False)
    for k, v in (("QOC_BLKSEG_S", S), ("QOC_BLKSEG_W", W), ("QOC_BLKSEG_PEN", segpen), ("QOC_BLKSEG_EXACT", segex)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    e.set_chain("taylor")
    if pen is not None:
        e.set_state_penalty(*pen)
    return e


def dev(u):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()


def bufs(B, Nt, nu):
    """J and dJdu on the device, NaN until the launch writes them."""
    import torch
    return (torch.full((B,), np.nan, dtype=torch.float64, device="cuda"),
            torch.full((B, Nt, nu), np.nan, dtype=torch.float64, device="cuda"))


def eval_dev(e, u, order=3):
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.eval_device(ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1))


def split_dev(e, u, order=3, check=None):
    """propagate then grape_sensitivity on device buffers; check(info) runs between the two."""
    B, nu, Nt = u.shape
    ud = dev(u)
    Jd, gd = bufs(B, Nt, nu)
    e.propagate_device(ud.data_ptr(), Jd.data_ptr())
    if check is not None:
        check(e.info())
    e.grape_sensitivity_device(ud.data_ptr(), order, gd.data_ptr())
    e.synchronize()
    return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1))


def assert_seed(J, g, Jr, gr, tag):
    rel = np.linalg.norm(g - gr) / np.linalg.norm(gr)
    print(tag, "dJ", J - Jr, "rel dJdu", rel)
    assert abs(J - Jr) <= 1e-12, (tag, J - Jr)
    assert rel <= 1e-10, (tag, rel)


def pen(p):
    return [int(r) for r in p[0]], [int(c) for c in p[1]], float(p[2])


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, controls, penalty) of the shipped systems."""
    from qoc_amd import systems
    if name == "zz":  # N = 9, 3 blocks of 3, m = 4, nu = 2; the reference's guard states |20>, |21>, |22>
        p = systems.zz_problem(60, tgate=6.0)
        qb = systems.QuantumBasis([3, 3])
        return p, systems.zz_controls(3, 60, 6.0, seed=81), (tuple(qb(["20", "21", "22"])), (0, 1, 2, 3), MU)
    if name == "cavity20":  # N = 20, 10 blocks of 2, m = 2
        p = systems.cavity_problem(N_cavity=10, Nt=50)
        return p, systems.cavity_controls(3, p.Nt, seed=82), ((16, 17, 18, 19, 5), (0, 1), MU)
    if name == "cavity40":  # N = 40 (the BASELINE system), 20 blocks of 2: the top two cavity levels of both qubit states
        p = systems.cavity_problem(N_cavity=20, Nt=77)
        return p, systems.cavity_controls(2, p.Nt, seed=83), ((18, 19, 38, 39), (0, 1), MU)
    raise KeyError(name)


def block_problem(NB, nblk, nu, m, Nt, seed, scale=1.0):
    """Random skew-Hermitian generators (exactly: -i H dt with H = (G + G^H) / 2) with nblk blocks of NB rows under a
    random permutation, the last block one row short (padding); scale raises every generator.  Returns the problem, the
    controls of two seeds and each block's rows in the permuted order."""
    from qoc_amd import systems
    rng = np.random.default_rng(seed)
    sizes = [NB] * (nblk - 1) + [NB - 1]
    N = sum(sizes)
    perm = rng.permutation(N)
    gens = []
    for j in range(nu + 1):
        H = np.zeros((N, N), complex)
        o = 0
        for s in sizes:
            G = rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))
            H[o:o + s, o:o + s] = (G + G.conj().T) / 2
            o += s
        H = H[np.ix_(perm, perm)]
        gens.append(-1j * H * (0.08 if j == 0 else 0.05) * scale)
    x0 = np.linalg.qr(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))[0]
    xt = np.linalg.qr(rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m)))[0]
    prob = systems.Problem("blocks", gens[0], gens[1:], x0, xt, float(m), Nt, "fp64")
    u = rng.uniform(-1, 1, size=(2, nu, Nt))
    inv = np.argsort(perm)  # row perm[i] of the block-ordered matrix sits at row i
    blocks, o = [], 0
    for s in sizes:
        blocks.append(sorted(int(inv[r]) for r in range(o, o + s)))
        o += s
    return prob, u, blocks
