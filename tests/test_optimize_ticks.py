"""Per-seed state machines (qoc_amd.optimize.minimize_ticks, the host reference of csrc/qoc_opt.hpp) against the
lock-step minimize_batched on the analytic problems of tests/test_optimize.py.  CPU only.

Seed by seed the two run the same algorithm, so the iterates agree to rounding; the per-seed schedule only stops
making every seed pay for the slowest seed's line search.  The comparisons stay away from the rounding floor of f,
where the Armijo test is decided by the last bit (bounded quadratic: gtol = 1e-6)."""
import ctypes

import numpy as np
import torch

from qoc_amd.optimize import minimize_batched, minimize_ticks

torch.set_default_dtype(torch.float64)


def rosen(x):
    a, c = x[:, 0], x[:, 1]
    f = (1 - a) ** 2 + 100 * (c - a * a) ** 2
    return f, torch.stack([-2 * (1 - a) - 400 * a * (c - a * a), 200 * (c - a * a)], 1)


ROSEN_X0 = torch.tensor([[-1.2, 1.0], [0.0, 0.0], [2.0, 2.0], [-0.5, 2.5]])


def quadratic(B=6, n=5):
    torch.manual_seed(0)
    Q = torch.randn(B, n, n)
    Q = Q @ Q.transpose(1, 2) + n * torch.eye(n)
    b = torch.randn(B, n) * 3

    def fg(x):
        r = torch.einsum("bij,bj->bi", Q, x)
        return 0.5 * (x * r).sum(1) - (b * x).sum(1), r - b
    return fg


def _counts(rt, rb):
    assert int(rt.evals.max()) <= rb.n_evals
    assert rt.ticks == int(rt.evals.max()) == rt.n_evals
    assert rt.not_done == 0 and bool(rt.done.all())
    assert rt.history == []


def test_rosenbrock_matches_lockstep():
    rb = minimize_batched(rosen, ROSEN_X0, max_iter=300)
    rt = minimize_ticks(rosen, ROSEN_X0, max_iter=300)
    assert float((rt.c - rb.c).abs().max()) <= 1e-12
    assert float((rt.f - rb.f).abs().max()) <= 1e-12
    assert torch.equal(rt.converged, rb.converged)
    _counts(rt, rb)
    # the schedule's gain: the slowest seed alone needs fewer evals than the lock-step batch
    assert rt.ticks < rb.n_evals


def test_sphere_augmented_lagrangian_matches_lockstep():
    cc = torch.tensor([[3.0, 4.0, 0.0], [0.1, 0.2, 0.3]])

    def fq(x):
        return ((x - cc) ** 2).sum(1), 2 * (x - cc)

    def cons(x):
        nrm = x.norm(dim=1, keepdim=True)
        return nrm, (x / nrm.clamp_min(1e-300))[:, None, :]
    kw = dict(cons=cons, g_upper=[1.0], max_iter=100, outer_iters=8)
    rb = minimize_batched(fq, torch.zeros_like(cc), **kw)
    rt = minimize_ticks(fq, torch.zeros_like(cc), **kw)
    assert float((rt.c - rb.c).abs().max()) <= 1e-12
    assert float((rt.f - rb.f).abs().max()) <= 1e-12
    assert float((rt.lam - rb.lam).abs().max()) <= 1e-12
    assert float((rt.g - rb.g).abs().max()) <= 1e-12
    assert rt.rounds.tolist() == [8, 8]
    _counts(rt, rb)


def test_bounded_quadratic_matches_lockstep():
    fg = quadratic()
    kw = dict(lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6)
    rb = minimize_batched(fg, torch.zeros(6, 5), **kw)
    rt = minimize_ticks(fg, torch.zeros(6, 5), **kw)
    assert float((rt.c - rb.c).abs().max()) <= 1e-9
    assert bool(rt.converged.all()) and float(rt.c.abs().max()) <= 0.5
    _counts(rt, rb)


def test_max_ticks_below_the_need():
    rt = minimize_ticks(rosen, ROSEN_X0, lower=-3.0, upper=3.0, max_iter=300, max_ticks=7)
    assert rt.ticks == 7 and rt.not_done == 4 and not bool(rt.done.any())
    assert rt.evals.tolist() == [7, 7, 7, 7]
    assert float(rt.c.abs().max()) <= 3.0
    # a seed that finishes stops counting: the quadratic's seeds need different numbers of evals
    fg = quadratic()
    full = minimize_ticks(fg, torch.zeros(6, 5), lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6)
    cut = int(full.evals.min()) + 1
    assert cut < full.ticks
    part = minimize_ticks(fg, torch.zeros(6, 5), lower=-0.5, upper=0.5, max_iter=200, gtol=1e-6, max_ticks=cut)
    assert part.evals.tolist() == [min(int(e), cut) for e in full.evals]
    assert part.not_done == int((full.evals > cut).sum()) > 0
    assert float(part.c.abs().max()) <= 0.5


def test_device_optimiser_envelope_is_refused_before_touching_the_gpu(built_lib):
    from qoc_amd import _lib
    h = ctypes.c_void_p()
    for n, mem in ((257, 10), (8, 17)):
        p = _lib.OptParams(n=n, ns=0, nu=0, lower=-1.0, upper=1.0, max_iter=5, memory=mem, outer_iters=1, max_ls=4,
                           rho0=10.0, gtol=1e-9, order=3)
        assert built_lib.qoc_opt_create(ctypes.byref(h), 0, 2, ctypes.byref(p)) == _lib.QOC_ERR_UNSUPPORTED
        assert not h.value and b"n <= 256" in built_lib.qoc_last_error(None)
    p = _lib.OptParams(n=8, ns=3, nu=2, lower=-1.0, upper=1.0, max_iter=5, memory=4, outer_iters=1, max_ls=4,
                       rho0=10.0, gtol=1e-9, order=3)
    assert built_lib.qoc_opt_create(ctypes.byref(h), 0, 2, ctypes.byref(p)) == _lib.QOC_ERR_ARG
