"""CPU: the cases of tests/opt_cases.py carry a device / host comparison of whole trajectories.

The device machine (csrc/qoc_opt.hpp) and the host reference (qoc_amd.optimize.minimize_ticks) see bit-identical f and
g and differ only in the order of their own sums (lane partials and a butterfly against numpy's sums).  Comparing
counts and iterates of whole runs means something only if no decision (Armijo, curvature, convergence, penalty raise)
hinges on the last bit of such a sum.  That condition is checked here on the reference alone: the variables are
permuted, fg and cons un-permute, evaluate and re-permute, so f and g stay bitwise those of the unpermuted problem and
only the machine's own sums change their order.  Every permuted run must take the same decisions and give the same
iterates within a tenth of the GPU test's bars (c 1e-10, f 1e-13 relative, lam 1e-7).  A case that fails this is
replaced, not loosened.

Each case is also asserted to reach what it is in the table for: the ring wraps, all 16 slots fill, no pair is ever
valid, three rounds end, the difference norm of ns = 1 is exactly 0."""
import numpy as np
import pytest
import torch

import opt_cases as OC
from qoc_amd import optimize
from qoc_amd.optimize import minimize_ticks

NPERM = 4


def _permuted(fn, perm, inv, grad_axis):
    def wrapped(y):
        a, b = fn(y[:, inv])
        return a, b.index_select(grad_axis, perm)
    return wrapped


@pytest.fixture(scope="module")
def host_runs():
    """The unpermuted host run of every case, once."""
    return {c.name: minimize_ticks(c.make("cpu"), c.c0(), **c.host_kw()) for c in OC.CASES}


@pytest.mark.parametrize("name", list(OC.BY_NAME))
def test_no_decision_hinges_on_the_order_of_a_sum(host_runs, name):
    case = OC.BY_NAME[name]
    ref = host_runs[name]
    fg = case.make("cpu")
    f0 = fg(case.c0())[0]
    scale = torch.maximum(ref.f.abs(), f0.abs())
    rng = np.random.default_rng(1000 + case.n)
    worst = [0.0, 0.0, 0.0]
    for _ in range(NPERM):
        perm = torch.from_numpy(rng.permutation(case.n))
        inv = torch.argsort(perm)
        kw = case.host_kw()
        if "cons" in kw:
            kw["cons"] = _permuted(kw["cons"], perm, inv, 2)
        # c0 = 0 is its own permutation
        r = minimize_ticks(_permuted(fg, perm, inv, 1), case.c0(), **kw)
        for k in ("evals", "iters", "ls_fails", "rounds", "converged"):
            assert getattr(r, k).tolist() == getattr(ref, k).tolist(), k
        assert r.ticks == ref.ticks and r.not_done == ref.not_done == 0
        worst[0] = max(worst[0], float((r.c[:, inv] - ref.c).abs().max()))
        worst[1] = max(worst[1], float(((r.f - ref.f).abs() / scale).max()))
        if ref.lam is not None:
            assert torch.equal(r.rho, ref.rho)
            worst[2] = max(worst[2], float((r.lam - ref.lam).abs().max()))
    print(f"{name}: max |dc| = {worst[0]:.3e}, rel |df| = {worst[1]:.3e}, |dlam| = {worst[2]:.3e}, "
          f"evals {ref.evals.tolist()}, iters {ref.iters.tolist()}")
    assert worst[0] <= 1e-10 and worst[1] <= 1e-13 and worst[2] <= 1e-7


@pytest.mark.parametrize("name", list(OC.BY_NAME))
def test_case_reaches_what_it_is_for(host_runs, name):
    case, ref = OC.BY_NAME[name], host_runs[name]
    reach = case.reach
    if "iters_at_least" in reach:  # the ring wraps (memory 1, 2, 10) or fills its 16 slots
        assert int(ref.iters.min()) >= reach["iters_at_least"]
        assert int(ref.ls_fails.max()) == 0  # no restart empties the ring on the way
    if name == "diagonal_n1_m10":
        # dg = [1] and |t| < 1: the scaled first step lands on the minimum, the second eval finds the gradient zero
        assert bool(ref.converged.all()) and ref.evals.tolist() == [2, 2, 2] and ref.iters.tolist() == [1, 1, 1]
    if "rounds" in reach:
        assert ref.rounds.tolist() == [reach["rounds"]] * case.B
        assert float(ref.lam.max()) > 0  # a constraint is active
    if case.ns == 1:
        assert ref.g[:, 1].tolist() == [0.0] * case.B and ref.lam[:, 1].tolist() == [0.0] * case.B
    if case.ns:
        g0 = optimize.spline_constraints_torch(case.c0(), case.ns, case.nu)[0]
        assert g0[:, 0].tolist() == [0.0] * case.B  # the first eval is at a zero norm


def test_table_is_the_one_the_counts_were_taken_on(host_runs):
    """The counts this table was built on; a change of a case shows here first."""
    for n in (63, 64, 65, 128, 129, 192, 193, 255, 256):
        r = host_runs[f"diagonal_n{n}_m10"]
        assert r.iters.tolist() == [24] * 3 and 25 <= int(r.evals.min()) and int(r.evals.max()) <= 28
        assert not bool(r.converged.any())
    for m in (1, 2, 16):
        r = host_runs[f"diagonal_n130_m{m}"]
        assert r.iters.tolist() == [24] * 3
    r = host_runs["linear_box"]
    assert bool(r.converged.all()) and float((r.c.abs() - 0.5).abs().max()) == 0.0  # every variable on a bound
    assert r.evals.tolist() == [5, 4] and r.iters.tolist() == [4, 3]
    for ns, nu in ((33, 3), (1, 5), (70, 1), (10, 2), (64, 4)):
        r = host_runs[f"constrained_ns{ns}_nu{nu}"]
        assert r.iters.tolist() == [24, 24] and 29 <= int(r.evals.min()) and int(r.evals.max()) <= 33


def test_linear_case_never_stores_a_pair(monkeypatch):
    """y = 0 exactly, so every accept takes the curvature skip (valid &= ~(1u << head) in opt_tell): after no accept
    is any pair valid, and there are accepts."""
    accepts = []

    class Recording(optimize._Seed):
        def tell(self, f, gr, gv, gj):
            before = self.iters
            super().tell(f, gr, gv, gj)
            if self.iters > before:
                accepts.append(bool(self.valid.any()))

    monkeypatch.setattr(optimize, "_Seed", Recording)
    case = OC.BY_NAME["linear_box"]
    r = minimize_ticks(case.make("cpu"), case.c0(), **case.host_kw())
    assert len(accepts) == int(r.iters.sum()) > 0
    assert not any(accepts)
    assert int(r.iters.min()) >= 2  # the skip runs with a history position to clear more than once per seed
