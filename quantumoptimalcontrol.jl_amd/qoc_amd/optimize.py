"""Batched multi-start optimiser over the spline coefficients — the caller of the batch axis
 and the stand-in for Ipopt in examples/zz_coupling_ipopt_exp.jl:56-80
(Ipopt itself is not available in this image).

B independent problems

    min_c  f(c)    s.t.   c_L <= c <= c_U,    g(c) <= g_U,     g(c) = [||c||, ||diff(c, dims=1)||]

advance in lock-step: every line-search trial is ONE batched f + grad evaluation of all seeds on
the GPU (``GrapeEngine.eval_spline_device``: u = transpose(Bs c), propagate, grape_sensitivity,
dJdc = Bs' dJdu').  Bounds are handled by projection (projected L-BFGS, Ipopt's
"hessian_approximation = limited-memory" analogue); the two norm constraints by an augmented
Lagrangian outer loop.  All vector work is batched torch on the engine's device; the optimiser
itself is generic over ``fg`` / ``cons`` callables, so the CPU tests drive it with analytic functions.

The lock-step is a scheduling choice: ``minimize_ticks`` runs the same algorithm as one state machine per seed (no
seed waits for another's line search), and ``minimize_on_device`` / ``DeviceOptimizer`` run those machines on the GPU
(csrc/qoc_opt.hpp) with no host decision between evals.

Variable layout: c is (B, nc) with nc = ns * nu in Julia's ``c[:]`` order of ``reshape(c, ns, nu)``
(index s + ns * j), which is also the engine's device layout.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


# ---------------------------------------------------------------------------------------------
# Objective / constraints on the engine
# ---------------------------------------------------------------------------------------------
class SplineGrape:
    """f + grad and the norm constraints of the Ipopt callbacks for B seeds on one GPU.

    Mirrors ``setup_ipopt_callbacks`` (examples/ipopt_callbacks_exp.jl:1-54): f(c) = Jfinal(x[end]) +
    sum(L, x) with u = transpose(B c); f_grad = B' transpose(dJdu); g = [norm(c), norm(diff(c))].
    """

    def __init__(self, engine, Bs, order: int = 3):
        import torch
        self.eng = engine
        self.order = order
        engine.set_spline_basis(Bs)
        self.ns, self.nu, self.B = engine.ns, engine.nu, engine.B
        self.nc = self.ns * self.nu
        self.device = torch.device("cuda", engine.device)
        self._J = torch.empty(self.B, dtype=torch.float64, device=self.device)
        self._G = torch.empty(self.B, self.nc, dtype=torch.float64, device=self.device)
        self._g = torch.empty(self.B, 2, dtype=torch.float64, device=self.device)
        self._gj = torch.empty(self.B, 2, self.nc, dtype=torch.float64, device=self.device)
        self.n_evals = 0

    def fg(self, c):
        import torch
        c = c.contiguous()
        torch.cuda.current_stream(self.device).synchronize()  # c produced on torch's stream
        self.eng.eval_spline_device(c.data_ptr(), self.order, self._J.data_ptr(), self._G.data_ptr())
        self.eng.synchronize()
        self.n_evals += 1
        return self._J.clone(), self._G.clone()

    def cons(self, c):
        import torch
        c = c.contiguous()
        torch.cuda.current_stream(self.device).synchronize()
        self.eng.spline_constraints_device(c.data_ptr(), self._g.data_ptr(), self._gj.data_ptr())
        self.eng.synchronize()
        return self._g.clone(), self._gj.clone()


class SplineGrapeDuration:
    """f + grad with the gate duration as one more variable per seed (``GrapeEngine.set_time_scale``), for the
    host-driven ``minimize_batched`` / ``minimize_ticks``, which take per-variable bounds.

    z = [c (ns * nu, SplineGrape's layout), τ] per seed, (B, ns * nu + 1);  f(z) = J(c; τ) + time_weight * τ and
    grad = [Bs' transpose(dJdu), dJ/dτ + time_weight].  J is the engine's at τ times the nominal duration, state
    penalty included; dJ/dτ is exact at every order.  Keep τ > 0 with a lower bound: the engine does not check values
    written to its device buffer.

    A device tensor z takes the device route: τ goes into the engine's own buffer (``time_scale_device``) and
    dJ/dτ is read from ``time_scale_grad_device``, so nothing crosses to the host that ``SplineGrape.fg`` does not
    move.  A host z (numpy or a CPU tensor) goes through ``set_time_scale`` / ``eval_spline`` / ``time_scale_grad``.
    """

    def __init__(self, engine, Bs, order: int = 3, time_weight: float = 0.0):
        self.eng = engine
        self.order = order
        self.kappa = float(time_weight)
        engine.set_spline_basis(Bs)
        self.ns, self.nu, self.B = engine.ns, engine.nu, engine.B
        self.nc = self.ns * self.nu
        self.n = self.nc + 1
        self.n_evals = 0
        self._dev = None

    def _device_buffers(self):
        import torch
        if not self.eng.time_scale_device():
            self.eng.set_time_scale(np.ones(self.B))
            self._dev = None
        if self._dev is None:
            dev = torch.device("cuda", self.eng.device)
            J = torch.empty(self.B, dtype=torch.float64, device=dev)
            G = torch.empty(self.B, self.nc, dtype=torch.float64, device=dev)
            tau = torch.as_tensor(_DevView(self.eng.time_scale_device(), (self.B,), "<f8"), device=dev)
            dtau = torch.as_tensor(_DevView(self.eng.time_scale_grad_device(), (self.B,), "<f8"), device=dev)
            self._dev = (dev, J, G, tau, dtau)
        return self._dev

    def fg(self, z):
        import torch
        self.n_evals += 1
        if isinstance(z, torch.Tensor) and z.is_cuda:
            dev, J, G, tau, dtau = self._device_buffers()
            c = z[:, :self.nc].contiguous()
            tau.copy_(z[:, self.nc])
            torch.cuda.current_stream(dev).synchronize()  # c and τ produced on torch's stream
            self.eng.eval_spline_device(c.data_ptr(), self.order, J.data_ptr(), G.data_ptr())
            self.eng.synchronize()
            return J + self.kappa * z[:, self.nc], torch.cat([G, (dtau + self.kappa)[:, None]], 1)
        zh = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z, dtype=np.float64)
        zh = zh.reshape(self.B, self.n)
        tau = zh[:, self.nc]
        self.eng.set_time_scale(tau)
        # c[s + ns j] is reshape(c, ns, nu)[s, j]: eval_spline takes and returns (B, ns, nu)
        J, dJdc = self.eng.eval_spline(np.transpose(zh[:, :self.nc].reshape(self.B, self.nu, self.ns), (0, 2, 1)), self.order)
        dtau = np.asarray(self.eng.time_scale_grad(), dtype=np.float64)
        g = np.concatenate([np.transpose(np.asarray(dJdc), (0, 2, 1)).reshape(self.B, self.nc),
                            (dtau + self.kappa)[:, None]], 1)
        return torch.from_numpy(np.asarray(J) + self.kappa * tau), torch.from_numpy(g)

    def cons(self, z):
        """The two spline norms of the c part and their (B, 2, n) Jacobian, whose τ column is zero: with ``fg`` the host
        reference of the constrained run, ``minimize_ticks(obj.fg, z0, lower=lo, upper=hi, cons=obj.cons, g_upper=...)``.
        A device z runs the engine's constraint kernel on the c part; a host z the torch form."""
        import torch
        if isinstance(z, torch.Tensor) and z.is_cuda:
            B, nc = self.B, self.nc
            c = z[:, :nc].contiguous()
            g = torch.empty(B, 2, dtype=torch.float64, device=z.device)
            gj = torch.empty(B, 2, nc, dtype=torch.float64, device=z.device)
            torch.cuda.current_stream(z.device).synchronize()
            self.eng.spline_constraints_device(c.data_ptr(), g.data_ptr(), gj.data_ptr())
            self.eng.synchronize()
            return g, torch.cat([gj, torch.zeros(B, 2, 1, dtype=torch.float64, device=z.device)], 2)
        zh = z if isinstance(z, torch.Tensor) else torch.from_numpy(np.asarray(z, dtype=np.float64))
        return duration_constraints_torch(zh.reshape(self.B, self.n), self.ns, self.nu)


def duration_constraints_torch(z, ns: int, nu: int):
    """``spline_constraints_torch`` on the c part of z = [c, τ] (B, ns * nu + 1); the Jacobian (B, 2, ns * nu + 1) has a
    zero τ column."""
    import torch
    nc = ns * nu
    g, gj = spline_constraints_torch(z[:, :nc], ns, nu)
    return g, torch.cat([gj, torch.zeros(z.shape[0], 2, 1, dtype=gj.dtype, device=gj.device)], 2)


def spline_constraints_torch(c, ns: int, nu: int):
    """Reference (torch) form of g = [norm(c), norm(diff(c, dims=1))] and its Jacobian (B, 2, nc)."""
    import torch
    B = c.shape[0]
    C = c.reshape(B, nu, ns).transpose(1, 2)  # (B, ns, nu) column-major per seed
    g0 = torch.linalg.vector_norm(c, dim=1)
    D = C[:, 1:, :] - C[:, :-1, :]
    g1 = torch.linalg.vector_norm(D.reshape(B, -1), dim=1)
    j0 = torch.where(g0[:, None] > 0, c / g0.clamp_min(1e-300)[:, None], torch.zeros_like(c))
    Dp = torch.zeros(B, ns + 1, nu, dtype=c.dtype, device=c.device)
    Dp[:, 1:ns, :] = D
    J1 = (Dp[:, :ns, :] - Dp[:, 1:, :])  # d_s - d_{s+1}
    j1 = J1.transpose(1, 2).reshape(B, -1)
    j1 = torch.where(g1[:, None] > 0, j1 / g1.clamp_min(1e-300)[:, None], torch.zeros_like(j1))
    return torch.stack([g0, g1], 1), torch.stack([j0, j1], 1)


# ---------------------------------------------------------------------------------------------
# Batched projected L-BFGS with an augmented-Lagrangian outer loop
# ---------------------------------------------------------------------------------------------
@dataclass
class BatchResult:
    c: object                 # (B, n) final iterates
    f: object                 # (B,) objective f (without constraint terms)
    g: object | None          # (B, ng) constraint values
    lam: object | None        # (B, ng) multipliers
    history: list = field(default_factory=list)   # per outer/inner iteration: f (B,) as numpy
    n_evals: int = 0
    converged: object = None  # (B,) bool


def _two_loop(q, S, Y, rho, valid, head, m):
    """H q for every seed from its L-BFGS pairs; S, Y (B, m, n), rho (B, m), valid (B, m) bool."""
    import torch
    B = q.shape[0]
    alpha = torch.zeros(B, m, dtype=q.dtype, device=q.device)
    q = q.clone()
    order = [(head - 1 - i) % m for i in range(m)]  # newest first
    for i in order:
        a = rho[:, i] * (S[:, i] * q).sum(1)
        a = torch.where(valid[:, i], a, torch.zeros_like(a))
        alpha[:, i] = a
        q = q - a[:, None] * Y[:, i]
    newest = order[0]
    sy = (S[:, newest] * Y[:, newest]).sum(1)
    yy = (Y[:, newest] * Y[:, newest]).sum(1)
    gamma = torch.where(valid[:, newest] & (yy > 0), sy / yy.clamp_min(1e-300), torch.ones_like(sy))
    r = gamma[:, None] * q
    for i in reversed(order):
        b = rho[:, i] * (Y[:, i] * r).sum(1)
        b = torch.where(valid[:, i], b, torch.zeros_like(b))
        r = r + (alpha[:, i] - b)[:, None] * S[:, i]
    return r


def minimize_batched(fg, c0, lower=None, upper=None, cons=None, g_upper=None, max_iter: int = 100,
                     memory: int = 10, outer_iters: int = 4, rho0: float = 10.0, gtol: float = 1e-9,
                     max_ls: int = 12, callback=None) -> BatchResult:
    """Minimise B independent problems in lock-step.

    fg(c) -> (f (B,), grad (B, n)); cons(c) -> (g (B, ng), jac (B, ng, n)) with constraints g <= g_upper.
    lower / upper: scalars or (n,) / (B, n) bounds.  max_iter counts inner iterations per outer round.
    """
    import torch
    x = c0.clone().to(torch.float64)
    B, n = x.shape
    dev = x.device
    lo = torch.full_like(x, -np.inf) if lower is None else torch.as_tensor(lower, dtype=x.dtype, device=dev).expand(B, n)
    hi = torch.full_like(x, np.inf) if upper is None else torch.as_tensor(upper, dtype=x.dtype, device=dev).expand(B, n)
    x = torch.minimum(torch.maximum(x, lo), hi)
    ng = 0
    if cons is not None:
        gu = torch.as_tensor(g_upper, dtype=x.dtype, device=dev).expand(B, -1)
        ng = gu.shape[1]
        lam = torch.zeros(B, ng, dtype=x.dtype, device=dev)
        rho = torch.full((B,), rho0, dtype=x.dtype, device=dev)
    evals = 0
    history = []

    def phi(xc):
        nonlocal evals
        f, gr = fg(xc)
        evals += 1
        if cons is None:
            return f, gr, f, None
        gv, gj = cons(xc)
        t = gv - gu
        a = torch.clamp(lam + rho[:, None] * t, min=0.0)
        pen = ((a * a) - lam * lam).sum(1) / (2 * rho)
        return f + pen, gr + torch.einsum("bi,bin->bn", a, gj), f, gv

    converged = torch.zeros(B, dtype=torch.bool, device=dev)
    fx = gxv = None
    for it_outer in range(max(1, outer_iters if cons is not None else 1)):
        fx, gx, f_true, gval = phi(x)
        S = torch.zeros(B, memory, n, dtype=x.dtype, device=dev)
        Y = torch.zeros_like(S)
        rh = torch.zeros(B, memory, dtype=x.dtype, device=dev)
        valid = torch.zeros(B, memory, dtype=torch.bool, device=dev)
        head = 0
        for it in range(max_iter):
            free = ~(((x <= lo) & (gx > 0)) | ((x >= hi) & (gx < 0)))
            q = gx * free
            pgn = q.abs().amax(1)
            converged = pgn <= gtol
            if bool(converged.all()):
                break
            d = -_two_loop(q, S, Y, rh, valid, head, memory) * free
            desc = (d * gx).sum(1)
            bad = ~(desc < 0)
            d = torch.where(bad[:, None], -q, d)
            valid = valid & ~bad[:, None]
            # first step of a fresh history: scaled steepest descent
            fresh = ~valid.any(1)
            step0 = torch.where(fresh, 1.0 / q.abs().amax(1).clamp_min(1e-12), torch.ones_like(pgn)).clamp(max=1.0)
            alpha = step0.clone()
            acc = converged.clone()
            x_new, f_new, g_new, ft_new, gv_new = x.clone(), fx.clone(), gx.clone(), f_true.clone(), gval
            for _ in range(max_ls):
                xt = torch.minimum(torch.maximum(x + alpha[:, None] * d, lo), hi)
                ft, gt, ftt, gvt = phi(xt)
                ok = (ft <= fx + 1e-4 * (gx * (xt - x)).sum(1)) & torch.isfinite(ft) & ~acc
                x_new = torch.where(ok[:, None], xt, x_new)
                f_new = torch.where(ok, ft, f_new)
                g_new = torch.where(ok[:, None], gt, g_new)
                ft_new = torch.where(ok, ftt, ft_new)
                if gvt is not None:
                    gv_new = torch.where(ok[:, None], gvt, gv_new)
                acc = acc | ok
                if bool(acc.all()):
                    break
                alpha = torch.where(acc, alpha, alpha * 0.5)
            s = x_new - x
            yv = g_new - gx
            sy = (s * yv).sum(1)
            upd = acc & ~converged & (sy > 1e-12 * s.norm(dim=1) * yv.norm(dim=1))
            S[:, head] = torch.where(upd[:, None], s, S[:, head])
            Y[:, head] = torch.where(upd[:, None], yv, Y[:, head])
            rh[:, head] = torch.where(upd, 1.0 / sy.where(upd, torch.ones_like(sy)), rh[:, head])
            valid[:, head] = torch.where(upd, torch.ones_like(upd), valid[:, head] & ~acc)
            head = (head + 1) % memory
            # seeds whose line search failed restart from steepest descent
            valid = valid & acc[:, None]
            x, fx, gx, f_true, gval = x_new, f_new, g_new, ft_new, gv_new
            history.append(f_true.detach().cpu().numpy().copy())
            if callback is not None:
                callback(it_outer, it, x, f_true)
        if cons is None:
            break
        t = gval - gu
        viol = t.clamp(min=0).amax(1)
        lam = torch.clamp(lam + rho[:, None] * t, min=0.0)
        if it_outer > 0:
            rho = torch.where(viol > 0.25 * prev_viol, rho * 10.0, rho)
        prev_viol = viol
    return BatchResult(c=x, f=f_true, g=gval, lam=lam if cons is not None else None, history=history,
                       n_evals=evals, converged=converged)


# ---------------------------------------------------------------------------------------------
# Per-seed state machines: the same algorithm with no seed waiting for another
# ---------------------------------------------------------------------------------------------
@dataclass
class TickResult(BatchResult):
    """BatchResult of a per-seed run.  n_evals is the tick count (batched evals); history stays empty."""
    evals: object = None      # (B,) evals each seed consumed before it was done
    iters: object = None      # (B,) accepted iterations
    rounds: object = None     # (B,) augmented-Lagrangian rounds ended
    ls_fails: object = None   # (B,) failed line searches
    done: object = None       # (B,) bool
    rho: object = None        # (B,) penalty
    ticks: int = 0
    not_done: int = 0


_INIT, _LS, _DONE = 0, 1, 2


class _Seed:
    """One seed's state machine (numpy, fp64): the per-seed semantics of ``minimize_batched``, quirks included.
    ``csrc/qoc_opt.hpp`` opt_tell runs the same rules on the device."""

    def __init__(self, x, lo, hi, ng, p):
        self.p = p
        self.lo, self.hi = lo, hi
        self.x = np.minimum(np.maximum(x, lo), hi)
        self.xt = self.x.copy()
        n, m = x.size, p["memory"]
        self.S, self.Y = np.zeros((m, n)), np.zeros((m, n))
        self.rinv = np.zeros(m)
        self.valid = np.zeros(m, dtype=bool)
        self.head = self.it = self.ls = self.round = 0
        self.lam = np.zeros(ng)
        self.rho = p["rho0"]
        self.prev_viol = 0.0
        self.phase = _INIT
        self.converged = False
        self.evals = self.iters = self.fails = 0
        self.fx = self.f_true = 0.0
        self.gx = np.zeros(n)
        self.gval = np.zeros(ng)
        self.d = np.zeros(n)
        self.alpha = 0.0

    def tell(self, f, gr, gv, gj):
        if self.phase == _DONE:
            return
        p = self.p
        self.evals += 1
        if gv is None:
            phi, gphi = f, gr
        else:
            t = gv - p["gu"]
            a = np.maximum(self.lam + self.rho * t, 0.0)
            phi = f + ((a * a) - self.lam * self.lam).sum() / (2 * self.rho)
            gphi = gr + (a[:, None] * gj).sum(0)
        if self.phase == _INIT:
            self._take(phi, gphi, f, gv)
            self.valid[:] = False
            self.head = self.it = 0
            return self._new_direction()
        xt, x = self.xt, self.x
        ok = bool(phi <= self.fx + 1e-4 * (self.gx * (xt - x)).sum()) and bool(np.isfinite(phi))
        m = p["memory"]
        if ok:
            s, y = xt - x, gphi - self.gx
            sy = (s * y).sum()
            upd = bool(sy > 1e-12 * np.sqrt((s * s).sum()) * np.sqrt((y * y).sum()))
            if upd:
                self.S[self.head], self.Y[self.head], self.rinv[self.head] = s, y, 1.0 / sy
            self.valid[self.head] = upd
            self.head = (self.head + 1) % m
            self.x = xt.copy()
            self._take(phi, gphi, f, gv)
            self.it += 1
            self.iters += 1
            return self._new_direction()
        self.ls += 1
        if self.ls == p["max_ls"]:  # the line search failed: steepest descent from x
            self.head = (self.head + 1) % m
            self.valid[:] = False
            self.it += 1
            self.fails += 1
            return self._new_direction()
        self.alpha *= 0.5
        self.xt = np.minimum(np.maximum(x + self.alpha * self.d, self.lo), self.hi)

    def _take(self, phi, gphi, f, gv):
        self.fx, self.gx, self.f_true = float(phi), np.array(gphi, dtype=np.float64), float(f)
        if gv is not None:
            self.gval = np.array(gv, dtype=np.float64)

    def _two_loop(self, q):
        m = self.p["memory"]
        order = [(self.head - 1 - i) % m for i in range(m)]  # newest first
        al = np.zeros(m)
        q = q.copy()
        for i in order:
            if self.valid[i]:
                al[i] = self.rinv[i] * (self.S[i] * q).sum()
                q = q - al[i] * self.Y[i]
        nw = order[0]
        gamma = 1.0
        if self.valid[nw]:
            yy = (self.Y[nw] * self.Y[nw]).sum()
            if yy > 0:
                gamma = (self.S[nw] * self.Y[nw]).sum() / yy
        r = gamma * q
        for i in reversed(order):
            if self.valid[i]:
                b = self.rinv[i] * (self.Y[i] * r).sum()
                r = r + (al[i] - b) * self.S[i]
        return r

    def _new_direction(self):
        p = self.p
        if self.it == p["max_iter"]:
            return self._end_round()
        x, gx = self.x, self.gx
        free = ~(((x <= self.lo) & (gx > 0)) | ((x >= self.hi) & (gx < 0)))
        q = gx * free
        pgn = np.abs(q).max()
        self.converged = bool(pgn <= p["gtol"])
        if self.converged:
            return self._end_round()
        d = -self._two_loop(q) * free
        if not (d * gx).sum() < 0:
            d = -q
            self.valid[:] = False
        self.alpha = 1.0 if self.valid.any() else min(1.0 / max(pgn, 1e-12), 1.0)
        self.d = d
        self.ls = 0
        self.xt = np.minimum(np.maximum(x + self.alpha * d, self.lo), self.hi)
        self.phase = _LS

    def _end_round(self):
        p = self.p
        self.xt = self.x.copy()
        if p["gu"] is None:
            self.round = 1
            self.phase = _DONE
            return
        t = self.gval - p["gu"]
        viol = np.maximum(t, 0.0).max()
        self.lam = np.maximum(self.lam + self.rho * t, 0.0)
        if self.round > 0 and viol > 0.25 * self.prev_viol:
            self.rho = self.rho * 10.0
        self.prev_viol = viol
        self.round += 1
        self.phase = _DONE if self.round >= max(1, p["outer_iters"]) else _INIT


def _default_max_ticks(max_iter, outer_iters, max_ls, constrained):
    return max(1, outer_iters if constrained else 1) * (1 + max_iter * max_ls)


def minimize_ticks(fg, c0, lower=None, upper=None, cons=None, g_upper=None, max_iter: int = 100, memory: int = 10,
                   outer_iters: int = 4, rho0: float = 10.0, gtol: float = 1e-9, max_ls: int = 12,
                   max_ticks: int | None = None) -> TickResult:
    """Host reference of the per-seed state machine, generic over ``fg`` / ``cons`` as
    ``minimize_batched`` is.  At every tick all B trial points are evaluated in one batched call and every seed
    consumes its own (f, grad): it accepts the trial and posts a new one, halves its step, or ends an
    augmented-Lagrangian round.  Seed by seed the iterates are ``minimize_batched``'s; no seed pays for another's
    line search.  Stops when every seed is done or after ``max_ticks`` ticks (``not_done`` tells which)."""
    import torch
    c0 = torch.as_tensor(c0).to(torch.float64)
    dev = c0.device
    X0 = c0.detach().cpu().numpy()
    B, n = X0.shape

    def bound(v, fill):
        if v is None:
            return np.full((B, n), fill)
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)
        return np.broadcast_to(v, (B, n)).astype(np.float64)
    lo, hi = bound(lower, -np.inf), bound(upper, np.inf)
    gu = None
    if cons is not None:
        gu = np.asarray(g_upper, dtype=np.float64)
        gu = np.broadcast_to(gu, (B, gu.shape[-1]))
    par = dict(max_iter=max_iter, memory=memory, outer_iters=outer_iters, rho0=rho0, gtol=gtol, max_ls=max_ls)
    seeds = [_Seed(X0[b], lo[b], hi[b], 0 if gu is None else gu.shape[1], dict(par, gu=None if gu is None else gu[b]))
             for b in range(B)]
    if max_ticks is None:
        max_ticks = _default_max_ticks(max_iter, outer_iters, max_ls, cons is not None)
    ticks = 0
    while ticks < max_ticks and any(s.phase != _DONE for s in seeds):
        xt = torch.from_numpy(np.stack([s.xt for s in seeds])).to(dev)
        f, gr = fg(xt)
        f, gr = f.detach().cpu().numpy(), gr.detach().cpu().numpy()
        gv = gj = None
        if cons is not None:
            gv, gj = cons(xt)
            gv, gj = gv.detach().cpu().numpy(), gj.detach().cpu().numpy()
        for b, s in enumerate(seeds):
            s.tell(f[b], gr[b], None if gv is None else gv[b], None if gj is None else gj[b])
        ticks += 1

    def T(a, dtype=None):
        return torch.from_numpy(np.asarray(a, dtype=dtype)).to(dev)
    return TickResult(
        c=T(np.stack([s.x for s in seeds])), f=T([s.f_true for s in seeds], np.float64),
        g=T(np.stack([s.gval for s in seeds])) if cons is not None else None,
        lam=T(np.stack([s.lam for s in seeds])) if cons is not None else None, history=[], n_evals=ticks,
        converged=T([s.converged for s in seeds], bool), evals=T([s.evals for s in seeds], np.int64),
        iters=T([s.iters for s in seeds], np.int64), rounds=T([s.round for s in seeds], np.int64),
        ls_fails=T([s.fails for s in seeds], np.int64), done=T([s.phase == _DONE for s in seeds], bool),
        rho=T([s.rho for s in seeds], np.float64) if cons is not None else None, ticks=ticks,
        not_done=sum(s.phase != _DONE for s in seeds))


class _DevView:
    """A device buffer owned by the library, exposed to torch through __cuda_array_interface__."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class DeviceOptimizer:
    """The per-seed state machines on the GPU (include/qoc.h qoc_opt_*; csrc/qoc_opt.hpp), as ask / tell:

        opt.start(c0); loop: f, grad at opt.trial -> opt.tell(f, grad); opt.result()

    Everything is queued on ``stream`` (default: torch's current stream on ``device``, so torch objectives need no
    synchronisation; pass ``engine.stream()`` to drive it with engine evals) and nothing waits for the host.
    ns, nu > 0 adds the spline-norm constraints g = [norm(c), norm(diff(c, dims=1))] <= g_upper, n = ns * nu.
    ``tau_bounds=(lo, hi)`` makes the duration form (qoc_opt_create_duration): the last variable is a gate duration with
    these bounds instead of lower / upper, left out of the constraints, and n = ns * nu + 1; ``time_weight`` is the κ of
    f = J + κ τ in ``GrapeEngine.minimize_spline_duration_device`` (ask / tell takes the caller's complete f and grad)."""

    def __init__(self, B: int, n: int, lower=None, upper=None, ns: int = 0, nu: int = 0, g_upper=None,
                 max_iter: int = 100, memory: int = 10, outer_iters: int = 4, rho0: float = 10.0, gtol: float = 1e-9,
                 max_ls: int = 12, order: int = 3, device: int = 0, stream: int | None = None, tau_bounds=None,
                 time_weight: float = 0.0):
        import ctypes as C
        from . import _lib as L
        from .engine import _order
        self._L, self._lib = L, L.load()
        gu = (0.0, 0.0) if g_upper is None else tuple(float(v) for v in g_upper)
        if ns and len(gu) != 2:
            raise ValueError("g_upper must hold the two spline-norm bounds")
        p = L.OptParams(n=int(n), ns=int(ns), nu=int(nu), lower=-np.inf if lower is None else float(lower),
                        upper=np.inf if upper is None else float(upper), g_upper=(C.c_double * 2)(*gu),
                        max_iter=int(max_iter), memory=int(memory), outer_iters=int(outer_iters), max_ls=int(max_ls),
                        rho0=float(rho0), gtol=float(gtol), order=_order(order))
        h = C.c_void_p()
        if tau_bounds is None:
            L.check(self._lib.qoc_opt_create(C.byref(h), int(device), int(B), C.byref(p)))
        else:
            d = L.OptDuration(tau_lower=float(tau_bounds[0]), tau_upper=float(tau_bounds[1]), time_weight=float(time_weight))
            L.check(self._lib.qoc_opt_create_duration(C.byref(h), int(device), int(B), C.byref(p), C.byref(d)))
        self._h = h
        self.B, self.n, self.device, self.constrained = int(B), int(n), int(device), bool(ns)
        self._stream = stream
        self.max_ticks = _default_max_ticks(max_iter, outer_iters, max_ls, bool(ns))
        self._trial = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.qoc_opt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _s(self):
        import ctypes as C
        if self._stream is not None:
            return C.c_void_p(self._stream)
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def start(self, c0):
        """c0: (B, n) float64 torch tensor on the device; the first trial is clamp(c0)."""
        import ctypes as C
        c0 = c0.contiguous()
        if tuple(c0.shape) != (self.B, self.n) or str(c0.dtype) != "torch.float64" or not c0.is_cuda:
            raise ValueError(f"c0 must be a float64 device tensor of shape {(self.B, self.n)}")
        self._keep = c0
        self._L.check(self._lib.qoc_opt_start_dev(self._h, self._s(), C.c_void_p(c0.data_ptr())))

    @property
    def trial(self):
        """(B, n) torch view of the trial points (the library's buffer, rewritten by every tell)."""
        if self._trial is None:
            import torch
            ptr = self._lib.qoc_opt_trial_dev(self._h)
            self._trial = torch.as_tensor(_DevView(ptr, (self.B, self.n), "<f8"), device=torch.device("cuda", self.device))
        return self._trial

    def trial_ptr(self) -> int:
        return int(self._lib.qoc_opt_trial_dev(self._h))

    def field_ptr(self, field: int) -> int:
        """Device pointer of a per-seed result (``_lib.QOC_OPT_*``)."""
        return int(self._lib.qoc_opt_field_dev(self._h, int(field)))

    def tell(self, f, grad):
        """f (B,), grad (B, n): float64 device tensors (or raw device pointers) at the current trials."""
        import ctypes as C
        if not isinstance(f, int):
            f, grad = f.contiguous(), grad.contiguous()
            self._keep_fg = (f, grad)
            f, grad = f.data_ptr(), grad.data_ptr()
        self._L.check(self._lib.qoc_opt_tell_dev(self._h, self._s(), C.c_void_p(f), C.c_void_p(grad)))

    def result(self, ticks: int | None = None) -> TickResult:
        """Waits for the stream and returns the per-seed results as torch tensors on the device."""
        import ctypes as C
        import torch
        B, n = self.B, self.n
        x, f, g, lam, rho = np.zeros((B, n)), np.zeros(B), np.zeros((B, 2)), np.zeros((B, 2)), np.zeros(B)
        ints = [np.zeros(B, dtype=np.int32) for _ in range(6)]
        nd = C.c_int()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        self._L.check(self._lib.qoc_opt_result(self._h, self._s(), *[a.ctypes.data_as(dp) for a in (x, f, g, lam, rho)],
                                               *[a.ctypes.data_as(ip) for a in ints], C.byref(nd)))
        evals, iters, rounds, conv, done, fails = ints
        dev = torch.device("cuda", self.device)

        def T(a, dtype=None):
            return torch.from_numpy(np.asarray(a, dtype=dtype)).to(dev)
        t = int(evals.max()) if ticks is None else int(ticks)
        return TickResult(c=T(x), f=T(f), g=T(g) if self.constrained else None, lam=T(lam) if self.constrained else None,
                          history=[], n_evals=t, converged=T(conv != 0), evals=T(evals, np.int64),
                          iters=T(iters, np.int64), rounds=T(rounds, np.int64), ls_fails=T(fails, np.int64),
                          done=T(done != 0), rho=T(rho) if self.constrained else None, ticks=t, not_done=int(nd.value))


def minimize_on_device(engine, Bs, c0, lower=None, upper=None, g_upper=None, max_iter: int = 100, memory: int = 10,
                       outer_iters: int = 4, rho0: float = 10.0, gtol: float = 1e-9, max_ls: int = 12, order: int = 3,
                       max_ticks: int | None = None, poll_every: int = 16) -> TickResult:
    """The multi-start optimisation of ``minimize_batched(SplineGrape(engine, Bs).fg, c0, ...)`` run on the GPU from
    start to finish (``GrapeEngine.minimize_spline_device``): per tick one eval and one fused step kernel on the
    engine's stream, the host only queues launches and polls a finished-seed count every ``poll_every`` ticks.
    ``g_upper = None`` leaves the two spline-norm constraints unbounded (one round).  Ends with a closing eval at the final iterates, so
    ``engine.allgather_best()`` is (min f, its seed).  ``history`` is empty; ``n_evals`` is the tick count."""
    import torch
    engine.set_spline_basis(Bs)
    ns, nu, B = engine.ns, engine.nu, engine.B
    dev = torch.device("cuda", engine.device)
    c = torch.as_tensor(c0).to(device=dev, dtype=torch.float64).reshape(B, ns * nu).clone().contiguous()
    torch.cuda.current_stream(dev).synchronize()  # c is produced on torch's stream
    if g_upper is None:
        g_upper, outer_iters = (np.inf, np.inf), 1
    opt = DeviceOptimizer(B, ns * nu, lower, upper, ns=ns, nu=nu, g_upper=g_upper, max_iter=max_iter, memory=memory,
                          outer_iters=outer_iters, rho0=rho0, gtol=gtol, max_ls=max_ls, order=order,
                          device=engine.device, stream=engine.stream())
    try:
        ticks = engine.minimize_spline_device(opt, c.data_ptr(), opt.max_ticks if max_ticks is None else max_ticks,
                                              poll_every)
        return opt.result(ticks)
    finally:
        opt.close()


def minimize_duration_on_device(engine, Bs, z0, lower, upper, tau_bounds, time_weight: float,
                                g_upper=None, max_iter: int = 100, memory: int = 10, outer_iters: int = 4,
                                rho0: float = 10.0, gtol: float = 1e-9, max_ls: int = 12, order: int = 3,
                                max_ticks: int | None = None, poll_every: int = 16) -> TickResult:
    """Time-optimal control on the GPU from start to finish: ``minimize_on_device`` over z = [c, τ] (B, ns * nu + 1) with
    f = J(c; τ) + time_weight * τ (``GrapeEngine.minimize_spline_duration_device``), seed by seed the run of
    ``minimize_ticks(SplineGrapeDuration(engine, Bs, order, time_weight).fg, z0, ...)`` with per-variable bounds.
    lower / upper bound c, ``tau_bounds`` τ; g_upper bounds the two spline norms of c (None: unbounded, one round).  A time
    scale of ones is set first when none is set; on return the engine's time scale holds the final τ, ``result.c`` the
    final z, ``result.f`` is J + time_weight * τ and ``engine.allgather_best()`` is (min J, its seed) of the closing eval."""
    import torch
    engine.set_spline_basis(Bs)
    ns, nu, B = engine.ns, engine.nu, engine.B
    if not engine.time_scale_device():
        engine.set_time_scale(np.ones(B))
    dev = torch.device("cuda", engine.device)
    z = torch.as_tensor(z0).to(device=dev, dtype=torch.float64).reshape(B, ns * nu + 1).clone().contiguous()
    torch.cuda.current_stream(dev).synchronize()  # z is produced on torch's stream
    if g_upper is None:
        g_upper, outer_iters = (np.inf, np.inf), 1
    opt = DeviceOptimizer(B, ns * nu + 1, lower, upper, ns=ns, nu=nu, g_upper=g_upper, max_iter=max_iter, memory=memory,
                          outer_iters=outer_iters, rho0=rho0, gtol=gtol, max_ls=max_ls, order=order,
                          device=engine.device, stream=engine.stream(), tau_bounds=tau_bounds, time_weight=time_weight)
    try:
        ticks = engine.minimize_spline_duration_device(opt, z.data_ptr(), opt.max_ticks if max_ticks is None else max_ticks,
                                                       poll_every)
        return opt.result(ticks)
    finally:
        opt.close()
