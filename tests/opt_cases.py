"""The shared case table of the optimiser shape tests: tests/test_optimize_cases_algebra.py checks on the CPU that every
case carries a device / host comparison, tests/test_gpu_optimize_shapes.py runs the cases on the device.

The objectives are elementwise torch with the row sums spelled out (as tests/test_gpu_optimize_device.py does), every
product and sum its own torch op: f and g of a seed do not depend on the batch, and the CPU and the GPU give the same
bits.  The host reference (qoc_amd.optimize.minimize_ticks) and the device machine (csrc/qoc_opt.hpp) therefore see
bit-identical f and g for identical trials and differ only in the order of their own sums.

What the shapes are for (csrc/qoc_opt.hpp opt_tell: lane l holds variables l, l + 64, l + 128, l + 192):
  diagonal n = 1 .. 256    every register-row boundary (64/65, 128/129, 192/193), rows 2 and 3, the full n = 256
  diagonal n = 130, m      the history ring at memory 1, 2 (head wraps at once) and 16 (the valid bit of slot 15)
  linear on a box          y = 0 on every accept: the curvature skip, no pair is ever valid
  constrained (ns, nu)     xt[r] - xtb[i - 1], xtb[i + 1] - xt[r] and i % ns across lanes and rows: ns not dividing
                           64, a column boundary on the lane 63 -> row 1 step (ns = 64), ns = 1 (the difference norm
                           is 0 by construction) and nu = 1 with n > 64
"""
from dataclasses import dataclass, field

import torch


def rowsum(a):
    acc = a[:, 0]
    for i in range(1, a.shape[1]):
        acc = acc + a[:, i]
    return acc


def diagonal(n, B=3, seed=3, device="cpu", sel=slice(None)):
    """f = 0.5 sum_i dg_i (x_i - t_i)^2: dg = linspace(1, 25, n), t = randn(B, n) of the given seed; sel picks seeds."""
    torch.manual_seed(seed)
    dg = torch.linspace(1, 25, n, dtype=torch.float64).to(device)
    tt = torch.randn(B, n, dtype=torch.float64)[sel].to(device)

    def fg(x):
        r = x - tt
        g = dg * r
        return 0.5 * rowsum(g * r), g
    return fg


def linear(device="cpu"):
    """f = b . x on a box: the gradient is constant, so y = 0 exactly on every accepted step."""
    b = torch.tensor([[1.5, -0.75, 0.5, -2.0, 0.25, 1.0, -0.1875],
                      [-0.5, 1.0, 2.0, -0.25, 0.5, -1.0, 1.0]], dtype=torch.float64).to(device)

    def fg(x):
        return rowsum(b * x), b + 0.0 * x
    return fg


@dataclass
class Case:
    name: str
    make: object              # make(device, sel=slice(None)) -> fg
    B: int
    n: int
    kw: dict                  # minimize_ticks / DeviceOptimizer settings
    ns: int = 0               # > 0: the spline-norm constraints on reshape(c, ns, nu)
    nu: int = 0
    reach: dict = field(default_factory=dict)  # what the host run must reach (test_optimize_cases_algebra.py)

    def c0(self, device="cpu"):
        return torch.zeros(self.B, self.n, dtype=torch.float64, device=device)

    def host_kw(self):
        """Settings of minimize_ticks: the constraints as the torch reference form."""
        from qoc_amd.optimize import spline_constraints_torch
        if not self.ns:
            return dict(self.kw)
        ns, nu = self.ns, self.nu
        return dict(self.kw, cons=lambda c: spline_constraints_torch(c, ns, nu))

    def device_kw(self):
        """Settings of DeviceOptimizer: it computes the constraints itself from (ns, nu)."""
        return dict(self.kw, ns=self.ns, nu=self.nu) if self.ns else dict(self.kw)


def _diag_case(n, memory):
    kw = dict(lower=-1.0, upper=1.0, max_iter=24, memory=memory, gtol=1e-6)
    reach = {} if n == 1 else dict(iters_at_least=16 if memory == 16 else memory + 1)  # fills / wraps
    return Case(f"diagonal_n{n}_m{memory}", lambda device, sel=slice(None), n=n: diagonal(n, 3, 3, device, sel), 3, n,
                kw, reach=reach)


def _cons_case(ns, nu):
    n = ns * nu
    kw = dict(lower=-1.0, upper=1.0, g_upper=[1.5, 0.8], max_iter=8, outer_iters=3)
    return Case(f"constrained_ns{ns}_nu{nu}", lambda device, sel=slice(None), n=n: diagonal(n, 2, 7, device, sel), 2, n,
                kw, ns=ns, nu=nu, reach=dict(rounds=3))


CASES = ([_diag_case(n, 10) for n in (1, 63, 64, 65, 128, 129, 192, 193, 255, 256)]
         + [_diag_case(130, m) for m in (1, 2, 16)]
         + [Case("linear_box", lambda device, sel=slice(None): linear(device), 2, 7,
                 dict(lower=-0.5, upper=0.5, max_iter=30), reach=dict(no_pairs=True))]
         + [_cons_case(ns, nu) for ns, nu in ((33, 3), (1, 5), (70, 1), (10, 2), (64, 4))])
BY_NAME = {c.name: c for c in CASES}
