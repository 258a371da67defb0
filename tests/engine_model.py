"""A stateless model of one live engine context, the op sequences drawn against it and the runner that applies a
sequence to a GrapeEngine and to the model side by side (tests/test_gpu_call_sequences.py).

The model holds the current settings (names into a System's tables) and three snapshots, nothing else.  The engine
keeps one record of qoc_ctx per snapshot (csrc/qoc_internal.hpp), named beside each:

    fwd   the controls (or spline coefficients), the settings and the call form of the last successful propagate /
          eval; None after anything that clears the engine's fwd.valid.
          LastFwd fwd: valid; kind (what a propagate left for the split sensitivity), lazy (x_k rebuilt on demand),
          captured, ichain / nwb / interp (the block-propagator forward's leftovers), steps_old / steps_cheb (the step
          records), formed_D / formed_ichain (report only); the host copies h_u, h_coef for the stale check (coef_ok)
    bwd   the forward it ran on, the settings at that time, the order and lambda_final of the last successful
          sensitivity / eval.
          LastBwd bwd: is_mu (d_L holds mu_k), lazy (lambda_k rebuilt on demand), route (info()["backward"])
    jfwd  the forward whose J the engine's J buffer still holds (setters do not clear it): allgather_best.
          LastJ jbest: ready (the eval already found the best pair), direct (and wrote it out)

"set" below is the record assigned plain (c->fwd = {}, c->bwd = {}) and then filled by the path that ran; "cleared" is
fwd.valid = false; "kept" may still be a targeted downgrade that leaves the values the same (set_state_penalty turns
fwd.kind 1 into 0: the sensitivity rebuilds x_k).

Every value is the oracle's (oracle/qoc_oracle.py) from scratch on a snapshot, memoised on the names.  The contract,
from include/qoc.h and, where the header is silent, csrc/qoc_engine.hip.  A NEW CACHED QUANTITY OF THE ENGINE BELONGS IN
THIS TABLE: which calls fill it, which calls must drop it.

    call                         fwd                 bwd      prediction
    ---------------------------  ------------------  -------  ------------------------------------------------------
    set_generators (new values)  cleared             kept     ok (the wrapper skips the call for bitwise equal values)
    set_x0, set_cost             cleared             kept     ok
    set_state_penalty            kept                kept     ok; J of a propagate is the penalty's of that propagate,
                                                              a later sensitivity runs on fwd's states with the current
                                                              penalty
    set_costate_source           kept                kept     ok; as the penalty, J never carries it
    set_spline_basis             kept, coefficients  kept     ok; sensitivity_spline is stale until the next
                                 forgotten                    propagate_spline
    comm_init(1, 0, None, off)   kept                kept     ok; allgather_best counts seeds from off
    eval_device                  set                 set      STATE under QOC_COST_EXTERNAL, else J and dJdu
    propagate, propagate_device  set                 kept     J (EXTERNAL: the penalty's sum alone)
    propagate_spline             set, coefficients   kept     J
                                 remembered
    eval_spline                  set, no             set      STATE under EXTERNAL (and the context untouched), else J, dJdc;
                                 coefficients                 the header promises sensitivity_spline for propagate_spline's
                                                              coefficients only, and the code agrees
    grape_sensitivity (host)     kept                set      STATE without fwd; STALE unless u is bitwise fwd's u and fwd
                                                              is no spline call; ARG under EXTERNAL without lambda_final;
                                                              else dJdu on fwd's states with the current penalty / source
    grape_sensitivity_device     kept                set      STATE without fwd or under EXTERNAL; STALE as above (the
                                                              caller's buffer is not written)
    sensitivity_spline           kept                set      STALE without fwd or unless fwd is a propagate_spline of
                                                              bitwise these coefficients under this basis; then STATE
                                                              under EXTERNAL
    state(k, seed)               -                   -        STATE without fwd, else fwd's x_k
    costate(k, seed)             -                   -        bwd's lambda_k under bwd's settings, whatever was set or
                                                              propagated since (zeros before the first sensitivity: the
                                                              generator does not ask)
    allgather_best               -                   -        (min J, off + argmin) of jfwd's J, lowest seed on ties

After a predicted error the model is unchanged and the context behaves as if the call had not been made.
"""
import functools
import os
import pprint
import sys
from collections import namedtuple

import numpy as np

if __name__ == "__main__":  # run as a script (pinned_routes): the import paths tests/conftest.py sets under pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "quantumoptimalcontrol.jl_amd"), os.path.join(_root, "oracle")]

import qoc_oracle as O  # noqa: E402

B = 3
ORDERS = (1, 3, 4, "exact")
STALE_MSG = "Cache data from other control signal u"
ERR_ARG, ERR_STALE, ERR_STATE = -1, -3, -4
SYSTEMS = ("cavity20", "zz", "tunable_bus", "tunable_bus_cz", "cavity_dense")

Settings = namedtuple("Settings", "gen x0 cost pen src basis offset")
Fwd = namedtuple("Fwd", "ctrl spline st coef_ok")
Bwd = namedtuple("Bwd", "fwd st order lam")


# ----------------------------------------------------------------------------------------------------------------------
# Systems: tables of named settings
# ----------------------------------------------------------------------------------------------------------------------
class System:
    def __init__(self, name, prob, fast=None):
        self.name, self.Nt, self.N, self.m, self.nu = name, prob.Nt, prob.N, prob.m, prob.nu
        self.gens = {"g0": (prob.A0, list(prob.A))}
        self.x0s = {"x0": (prob.x0, False)}
        self.costs = {"trace": ("trace", prob.x_target, prob.n), "trace_neg": ("trace", -prob.x_target, prob.n),
                      "ext": ("ext", None, 1.0)}
        self.pens = {"off": ((), (), 0.0)}
        self.srcs, self.lams, self.ctrls, self.bases, self.coefs = {}, {}, {}, {}, {}
        self.fast = fast          # info()["backward"] of the system's fast path, None: none asserted
        self.blocks = None        # row lists of the invariant blocks whose liveness the engine tracks
        rng = np.random.default_rng(sum(map(ord, name)))
        shape = (B, self.Nt + 1, self.N, self.m)
        self.srcs["src0"] = 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
        self.lams["lam0"] = rng.standard_normal((B, self.N, self.m)) + 1j * rng.standard_normal((B, self.N, self.m))
        self.rng = rng

    def per_seed_x0(self):
        """x0 with another phase and weight per seed and column: the same support, so the same live blocks."""
        x0 = self.x0s["x0"][0]
        f = self.rng.uniform(0.5, 1.0, size=(B, 1, self.m)) * np.exp(1j * self.rng.uniform(-3, 3, size=(B, 1, self.m)))
        self.x0s["x0_seed"] = (x0[None] * f, True)

    def compatible(self, x0, cost):
        """False where x0 and the target share no block: J = 1 and dJdu = 0 exactly, nothing to compare against."""
        kind, xt, _ = self.costs[cost]
        if self.blocks is None or kind == "ext":
            return True
        x = self.x0s[x0][0]
        x = np.abs(x).sum(axis=0) if x.ndim == 3 else np.abs(x)
        return any(x[rows].any() and np.abs(xt[rows]).any() for rows in self.blocks)

    def dead_rows(self, x0, cost):
        """Rows of the blocks that carry neither x0 nor the target (csrc/qoc_run_blk.hip blk_live_rows)."""
        kind, xt, _ = self.costs[cost]
        if self.blocks is None or kind == "ext":
            return []
        x = self.x0s[x0][0]
        x = np.abs(x).sum(axis=0) if x.ndim == 3 else np.abs(x)
        return [r for rows in self.blocks if not (x[rows].any() or np.abs(xt[rows]).any()) for r in rows]

    def ctrl(self, name):
        """A control or coefficient array by name; a trailing * is the same array with one entry moved by 1e-9."""
        base = name.rstrip("*")
        a = self.ctrls[base] if base in self.ctrls else self.coefs[base]
        if name.endswith("*"):
            a = a.copy()
            a[1, 0, 5 % a.shape[2]] += 1e-9
        return a


def _mixed(u, amps):
    """Seed b of u scaled by amps[b]: the seeds of one launch in different series classes."""
    return u * np.asarray(amps, dtype=float)[:, None, None]


@functools.lru_cache(maxsize=None)
def system(name):
    from qoc_amd import systems
    import blkseg_util
    if name == "cavity20":  # N = 20, 10 blocks of 2 rows; Nt = 43: an odd last segment (tests/test_gpu_blkseg_peel.py)
        p = systems.cavity_problem(N_cavity=10, Nt=43)
        s = System(name, p, fast="segmented")
        p7 = systems.cavity_problem(N_cavity=10, Nt=43, dt=0.7)
        pb, _, _ = blkseg_util.block_problem(3, 7, 2, 2, 43, seed=77)  # N = 20 again: 6 blocks of 3 rows and one of 2
        s.gens.update(g_dt=(p7.A0, list(p7.A)), g_blk3=(pb.A0, list(pb.A)),
                      g_inexact=(p.A0 + 1e-14 * np.abs(p.A0).max() * np.eye(p.N), list(p.A)))
        s.x0s["x0_blk"] = (pb.x0, False)
        s.costs["trace_blk"] = ("trace", pb.x_target, pb.n)
        s.pens.update(pen0=((16, 17, 18, 19, 5), (0, 1), blkseg_util.MU), pen1=((3, 12), (1,), 0.8),
                      mu0=((16, 17, 18, 19, 5), (0, 1), 0.0))
        # the series classes K = 5 / 7 / 9 and the halving amplitude of tests/test_gpu_blkseg_peel.py, mixed per seed
        for i, amps in enumerate([(1, 8, 14), (22, 1, 8), (14, 22, 1)]):
            s.ctrls[f"u{i}"] = _mixed(systems.cavity_controls(B, p.Nt, seed=700 + i), amps)
        s.ctrls["u3"] = 0.5 * s.ctrls["u0"]
    elif name == "zz":  # N = 9, 3 blocks of 3 rows, m = 4
        tg = 2.4
        p = systems.zz_problem(24, tgate=tg)
        s = System(name, p, fast="segmented")
        p2 = systems.zz_problem(24, tgate=3.6)
        qb = systems.QuantumBasis([3, 3])
        s.gens["g_dt"] = (p2.A0, list(p2.A))
        s.costs["zcal"] = ("zcal", p.x_target, 4.0)
        s.pens.update(pen0=(tuple(qb(["20", "21", "22"])), (0, 1, 2, 3), blkseg_util.MU),
                      pen1=(tuple(qb(["02", "12"])), (0, 2), 0.6), mu0=(tuple(qb(["20", "21", "22"])), (0, 1, 2, 3), 0.0))
        # the amplitudes of tests/test_gpu_blkseg_exact.py::test_exact_series_degree_classes_and_halving
        for i, amps in enumerate([(1, 8, 14), (22, 1, 8), (14, 22, 1)]):
            s.ctrls[f"u{i}"] = _mixed(systems.zz_controls(B, 24, tg, seed=710 + i, nsplines=6), amps)
        s.ctrls["u3"] = 0.5 * s.ctrls["u0"]
        Bs = systems.spline_matrix(tg, 24, 6)
        s.bases.update(bs=Bs, bs_half=0.5 * Bs)
        for i in range(2):
            s.coefs[f"c{i}"] = s.rng.uniform(-0.377, 0.377, size=(B, Bs.shape[1], 2)) * (1 + 7 * i)
    elif name in ("tunable_bus", "tunable_bus_cz"):  # N = 27, the parity blocks of 14 + 13 rows
        Nt = 21
        tg = 350.0 * Nt / 2000
        mk = systems.tunable_bus_problem if name == "tunable_bus" else systems.tunable_bus_cz_problem
        p = mk(Nt=Nt, tgate=tg)
        s = System(name, p, fast="blocks_prop16")
        s.blocks = [list(range(0, 27, 2)), list(range(1, 27, 2))]
        p2 = mk(Nt=Nt, tgate=0.8 * tg)
        s.gens["g_dt"] = (p2.A0, list(p2.A))
        qb = systems.QuantumBasis([3, 3, 3])
        rows = lambda labels: tuple(int(r) for r in qb(labels))  # noqa: E731
        base = systems.tunable_bus_controls(B, Nt, seed=720)     # in [0.3, 1.0]
        base2 = systems.tunable_bus_controls(B, Nt, seed=721)
        t = lambda u: (u - 0.3) / 0.7                             # noqa: E731
        # narrow: [0.45, 0.75]; wide: three times that range around it; flat: every slice equal, outside both
        s.ctrls.update(narrow=0.45 + 0.3 * t(base), narrow2=0.45 + 0.3 * t(base2), wide=0.15 + 0.9 * t(base),
                       flat=np.full((B, 1, Nt), 1.3))
        if name == "tunable_bus":
            s.pens.update(pen0=(rows(["020", "011", "002", "101", "010"]), (0,), 0.3),
                          pen1=(rows(["020", "101"]), (0,), 0.7), mu0=(rows(["020", "011", "002", "101", "010"]), (0,), 0.0))
            col = lambda *labels: (qb.columns(list(labels)).sum(axis=1, keepdims=True) / np.sqrt(len(labels))).astype(complex)  # noqa: E731
            s.x0s.update(x0_odd=(col("100"), False), x0_both=(col("110", "100"), False))
            s.costs.update(trace_odd=("trace", col("001"), 1.0), trace_both=("trace", col("200", "001"), 1.0))
            Bs = systems.spline_matrix(tg, Nt, 6)
            s.bases.update(bs=Bs, bs_half=0.5 * Bs)
            s.coefs.update(cn=s.rng.uniform(0.45, 0.75, size=(B, 6, 1)), cw=s.rng.uniform(0.15, 1.05, size=(B, 6, 1)))
        else:
            s.costs["zcal"] = ("zcal", p.x_target, 4.0)
            s.pens.update(pen0=(rows(["200", "020", "002", "110", "011"]), (0, 1, 3), 0.3),
                          pen1=(rows(["200", "011"]), (2,), 0.7), mu0=(rows(["200", "020", "002", "110", "011"]), (0, 1, 3), 0.0))
    elif name == "cavity_dense":  # no invariant blocks: the Taylor-action chains, captured products, concurrent backward
        p = systems.cavity_dense_problem(N_cavity=8, Nt=12)
        s = System(name, p)
        p2 = systems.cavity_dense_problem(N_cavity=8, Nt=12, dt=0.7)
        s.gens["g_dt"] = (p2.A0, list(p2.A))
        s.pens.update(pen0=((6, 7, 14, 15), (0, 1), 0.37), pen1=((3,), (1,), 0.8), mu0=((6, 7, 14, 15), (0, 1), 0.0))
        for i, amp in enumerate([1.0, 2.0, 0.5]):
            s.ctrls[f"u{i}"] = amp * systems.cavity_controls(B, p.Nt, seed=730 + i)
    else:
        raise KeyError(name)
    if name != "tunable_bus":
        s.per_seed_x0()
    for tab in (s.ctrls, s.coefs, s.srcs, s.lams):
        for a in tab.values():
            a.setflags(write=False)
    return s


def default_settings(s):
    return Settings("g0", "x0", "trace", "off", None, "bs" if s.bases else None, 0)


# ----------------------------------------------------------------------------------------------------------------------
# The oracle on a snapshot (memoised on the names)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def controls_of(sysname, ctrl, spline, basis):
    s = system(sysname)
    a = s.ctrl(ctrl)
    if not spline:
        return a
    Bs = s.bases[basis]
    return np.stack([(Bs @ a[b]).T for b in range(B)])  # u_b = transpose(Bs c_b)


@functools.lru_cache(maxsize=None)
def forward_of(sysname, gen, x0, ctrl, spline, basis):
    """The oracle's cache (x_k, U_k) of every seed."""
    s = system(sysname)
    A0, A = s.gens[gen]
    x, per_seed = s.x0s[x0]
    u = controls_of(sysname, ctrl, spline, basis)
    out = []
    for b in range(B):
        cache = O.setup_grape_cache(A0, x[b] if per_seed else x, u[b].shape)
        O.propagate(A0, A, u[b], x[b] if per_seed else x, cache)
        out.append(cache)
    return tuple(out)


def _fkey(f):
    return (f.st.gen, f.st.x0, f.ctrl, f.spline, f.st.basis if f.spline else None)


@functools.lru_cache(maxsize=None)
def J_of(sysname, fkey, cost, pen):
    s = system(sysname)
    kind, xt, n = s.costs[cost]
    P, C, mu = s.pens[pen]
    L = O.setup_state_penalty(P, C, mu)[0] if mu != 0.0 and len(P) and len(C) else None
    Jf = {"trace": lambda: O.setup_infidelity(xt, n)[0], "zcal": lambda: O.setup_infidelity_zcalibrated(xt)[0],
          "ext": lambda: (lambda x: 0.0)}[kind]()
    return np.array([Jf(c.x[-1]) + (sum(L(x) for x in c.x) if L else 0.0) for c in forward_of(sysname, *fkey)])


@functools.lru_cache(maxsize=None)
def backward_of(sysname, fkey, cost, pen, src, order, lam, dtheta=0.0):
    """(lambda_k (B, Nt+1, N, m), dJdu (B, nu, Nt)) of grape_sensitivity on the forward's states; dtheta moves the
    z-calibrated cost's calibration phase (qoc_oracle.setup_infidelity_zcalibrated_shifted)."""
    s = system(sysname)
    A0, A = s.gens[fkey[0]]
    kind, xt, n = s.costs[cost]
    P, C, mu = s.pens[pen]
    pen_dL = O.setup_state_penalty(P, C, mu)[1] if mu != 0.0 and len(P) and len(C) else None
    lams, grads = [], []
    for b, fc in enumerate(forward_of(sysname, *fkey)):
        if kind == "trace":
            dJ = O.setup_infidelity(xt, n)[1]
        elif kind == "zcal":
            dJ = O.setup_infidelity_zcalibrated_shifted(xt, dtheta)[1]
        else:
            dJ = (lambda lf: lambda x: lf)(s.lams[lam][b])
        dL = None
        if pen_dL is not None or src is not None:
            kof = {id(x): k for k, x in enumerate(fc.x)}  # the caller's closure, evaluated on the states: by slice

            def dL(x, kof=kof, b=b):
                g = pen_dL(x) if pen_dL is not None else np.zeros_like(x)
                return g + s.srcs[src][b, kof[id(x)]] if src is not None else g
        cache = O.GrapeCache(x=fc.x, lam=[None] * len(fc.x), dJdu=np.zeros_like(fc.u), Uk=fc.Uk, u=fc.u, degrees=fc.degrees)
        g = O.grape_sensitivity(A0, A, dJ, fc.u, None, cache, dUkdp_order=order, dL_dx=dL)
        lams.append(np.stack(cache.lam))
        grads.append(g.copy())
    return np.stack(lams), np.stack(grads)


# ----------------------------------------------------------------------------------------------------------------------
# Predictions
# ----------------------------------------------------------------------------------------------------------------------
class Pred:
    """What the model expects of one op: kind in ok / err / J / g / Jg / x / lam / best / unknown."""

    def __init__(self, kind, sysname, **kw):
        self.kind, self.sysname = kind, sysname
        self.__dict__.update(kw)

    def J(self):
        return J_of(self.sysname, _fkey(self.fwd), self.fwd.st.cost, self.fwd.st.pen)

    def _bkey(self):
        b = self.bwd
        return (_fkey(b.fwd), b.fwd.st.cost, b.st.pen, b.st.src, b.order, b.lam)

    def zcal(self):
        return system(self.sysname).costs[self.bwd.fwd.st.cost][0] == "zcal"

    def lam_g(self, dtheta=0.0):
        """bwd's co-states and gradient (in the coefficients for a spline call: dJdc_b = Bs' transpose(dJdu_b))."""
        lam, g = backward_of(self.sysname, *self._bkey(), dtheta)
        if getattr(self, "spline_grad", False):
            Bs = system(self.sysname).bases[self.bwd.fwd.st.basis]
            g = np.stack([Bs.T @ g[b].T for b in range(B)])
        return lam, g

    def states(self):
        return [np.stack(c.x) for c in forward_of(self.sysname, *_fkey(self.fwd))]

    def dtheta_bound(self, b):
        s = system(self.sysname)
        return O.zcal_dtheta_bound(s.costs[self.bwd.fwd.st.cost][1], forward_of(self.sysname, *_fkey(self.bwd.fwd))[b].x[-1])


class Model:
    def __init__(self, sysname):
        self.sysname = sysname
        self.s = system(sysname)
        self.st = default_settings(self.s)
        self.fwd = self.bwd = self.jfwd = None

    def _err(self, stale=False, code=ERR_STATE):
        return Pred("err", self.sysname, stale=stale, code=ERR_STALE if stale else code)

    def _stale(self, name, spline_call):
        f = self.fwd
        if spline_call:
            return not (f.spline and f.coef_ok and np.array_equal(self.s.ctrl(name), self.s.ctrl(f.ctrl)))
        return f.spline or not np.array_equal(self.s.ctrl(name), self.s.ctrl(f.ctrl))

    def apply(self, op):
        s, st, name = self.s, self.st, op[0]
        P = functools.partial(Pred, sysname=self.sysname)
        ext = s.costs[st.cost][0] == "ext"
        if name in ("set_gen", "set_x0", "set_cost"):
            field = name[4:]
            if name == "set_gen" and op[1] == st.gen:
                return P("ok")
            assert op[1] in getattr(s, field + "s"), op
            self.st = st._replace(**{field: op[1]})
            self.fwd = None
            return P("ok")
        if name in ("set_pen", "set_src", "set_basis"):
            self.st = st._replace(**{name[4:]: op[1]})
            if name == "set_basis" and self.fwd is not None:
                self.fwd = self.fwd._replace(coef_ok=False)
            return P("ok")
        if name == "comm":
            self.st = st._replace(offset=op[1])
            return P("ok")
        if name in ("eval", "eval_spl"):
            if ext:
                return self._err()
            self.fwd = self.jfwd = Fwd(op[1], name == "eval_spl", st, False)
            self.bwd = Bwd(self.fwd, st, op[2], None)
            return P("Jg", fwd=self.fwd, bwd=self.bwd, spline_grad=name == "eval_spl")
        if name in ("prop", "prop_dev", "prop_spl"):
            self.fwd = self.jfwd = Fwd(op[1], name == "prop_spl", st, name == "prop_spl")
            return P("J", fwd=self.fwd)
        if name in ("sens", "sens_dev", "sens_spl"):
            lam = op[3] if len(op) > 3 else None
            if name == "sens_spl":
                if self.fwd is None or self._stale(op[1], True):
                    return self._err(stale=True)
                if ext:
                    return self._err()
            else:
                if self.fwd is None or (name == "sens_dev" and ext):
                    return self._err()
                if self._stale(op[1], False):
                    return self._err(stale=True)
                if ext and lam is None:
                    return self._err(code=ERR_ARG)
            self.bwd = Bwd(self.fwd, st, op[2], lam if ext else None)
            return P("g", bwd=self.bwd, spline_grad=name == "sens_spl")
        if name in ("state", "state_dead0"):
            if self.fwd is None:
                return self._err()
            return P("x", fwd=self.fwd, k=op[1], seed=op[2],
                     zero_rows=s.dead_rows(self.fwd.st.x0, self.fwd.st.cost) if name == "state_dead0" else None)
        if name in ("costate", "costate_dead0"):
            if self.bwd is None:
                return P("unknown")
            f = self.bwd.fwd
            return P("lam", bwd=self.bwd, k=op[1], seed=op[2],
                     zero_rows=s.dead_rows(f.st.x0, f.st.cost) if name == "costate_dead0" else None)
        if name == "best":
            if self.jfwd is None:
                return P("unknown")
            return P("best", fwd=self.jfwd, offset=st.offset)
        raise KeyError(op)


# ----------------------------------------------------------------------------------------------------------------------
# Generated sequences
# ----------------------------------------------------------------------------------------------------------------------
SETTERS = ("set_pen", "set_src", "set_cost", "set_x0", "set_gen", "set_basis", "comm")
FOLLOWERS = ("eval", "propagate", "sensitivity", "state", "costate")
CALLS = ("eval", "propagate", "propagate_device", "sensitivity", "sensitivity_stale", "state", "costate", "best", "triple")
CALL_WEIGHTS = (0.2, 0.12, 0.12, 0.18, 0.1, 0.08, 0.08, 0.05, 0.07)


def setters_of(s):
    return tuple(c for c in SETTERS if c != "set_basis" or s.bases)


class _Deck:
    """Draws without replacement, reshuffled when empty: every item comes up once per round."""

    def __init__(self, rng, items):
        self.rng, self.items, self.left = rng, list(items), []

    def draw(self):
        if not self.left:
            self.left = [self.items[i] for i in self.rng.permutation(len(self.items))]
        return self.left.pop()


def gen_ops(sysname, seed, n=40):
    """n ops from default_rng: about a third setters, each followed by a call of a class its deck deals; the model runs
    along, so that a sensitivity can name the forward's own u (or miss it on purpose)."""
    s = system(sysname)
    rng = np.random.default_rng([SYSTEMS.index(sysname), seed])
    m = Model(sysname)
    ops = []
    setters = _Deck(rng, setters_of(s))
    follow = {c: _Deck(rng, FOLLOWERS) for c in SETTERS}
    values = {"set_pen": _Deck(rng, list(s.pens)), "set_src": _Deck(rng, [None, "src0"]),
              "set_cost": _Deck(rng, list(s.costs)), "set_x0": _Deck(rng, list(s.x0s)),
              "set_gen": _Deck(rng, list(s.gens)), "set_basis": _Deck(rng, list(s.bases) or [None])}
    pool = _Deck(rng, list(s.ctrls))
    cpool = _Deck(rng, list(s.coefs) or [None])
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731

    def emit(op):
        ops.append(op)
        assert m.apply(op).kind != "unknown", op

    def forward(cls):
        spl = bool(s.coefs) and cls != "propagate_device" and rng.random() < 0.25
        if cls == "eval":
            emit(("eval_spl", cpool.draw(), pick(ORDERS)) if spl else ("eval", pool.draw(), pick(ORDERS)))
        elif spl:
            emit(("prop_spl", cpool.draw()))
        else:
            emit(("prop" if cls == "propagate" else "prop_dev", pool.draw()))

    def call(cls):
        ext = s.costs[m.st.cost][0] == "ext"
        if cls in ("eval", "propagate", "propagate_device"):
            forward(cls)
        elif cls == "sensitivity":
            f = m.fwd
            order = pick(ORDERS)
            if f is not None and f.spline:
                emit(("sens_spl", f.ctrl, order))
            else:
                u = f.ctrl if f is not None else pool.draw()
                if ext or rng.random() < 0.5:
                    emit(("sens", u, order, "lam0") if ext else ("sens", u, order))
                else:
                    emit(("sens_dev", u, order))
        elif cls == "sensitivity_stale":
            f = m.fwd
            if f is None or f.spline:
                return call("propagate_device" if rng.random() < 0.5 else "propagate")
            u = f.ctrl.rstrip("*") + "*" if rng.random() < 0.6 or len(s.ctrls) < 2 else pick([c for c in s.ctrls if c != f.ctrl.rstrip("*")])
            if f.ctrl.endswith("*") and u == f.ctrl:
                u = f.ctrl.rstrip("*")
            emit(("sens", u, pick(ORDERS), "lam0") if ext else (pick(["sens", "sens_dev"]), u, pick(ORDERS)))
        elif cls in ("state", "costate"):
            if cls == "costate" and m.bwd is None:
                return call("eval" if not ext else "propagate")
            emit((cls, int(pick([0, s.Nt, s.Nt // 3, int(rng.integers(s.Nt + 1))])), int(rng.integers(B))))
        elif cls == "best":
            if m.jfwd is None:
                return call("propagate")
            emit(("best",))
        elif cls == "triple":  # an eval's co-states must survive a later propagate
            if ext:
                return call("propagate")
            forward("eval")
            call("propagate" if rng.random() < 0.5 else "propagate_device")
            call("costate")
        else:
            raise KeyError(cls)

    call("eval")  # a configured engine with one eval behind it
    while len(ops) < n:
        if rng.random() < 0.5:
            cls = setters.draw()
            emit(("comm", int(pick([0, 7, 1000]))) if cls == "comm" else (cls, values[cls].draw()))
            if not s.compatible(m.st.x0, m.st.cost):  # the other of x0 / target follows into the same block
                if cls == "set_x0":
                    emit(("set_cost", pick([c for c in s.costs if s.compatible(m.st.x0, c)])))
                else:
                    emit(("set_x0", pick([x for x in s.x0s if s.compatible(x, m.st.cost)])))
            else:
                call(follow[cls].draw())
        else:
            call(CALLS[int(rng.choice(len(CALLS), p=CALL_WEIGHTS))])
    return ops[:n]


def classify(sysname, ops):
    """The op classes of a sequence (a sensitivity the model predicts stale is a class of its own) and, per forward,
    the controls' names."""
    m = Model(sysname)
    names = {"eval": "eval", "eval_spl": "eval", "prop": "propagate", "prop_spl": "propagate", "prop_dev": "propagate_device",
             "state": "state", "state_dead0": "state", "costate": "costate", "costate_dead0": "costate", "best": "best"}
    out = []
    for op in ops:
        p = m.apply(op)
        if op[0].startswith("sens"):
            out.append("sensitivity_stale" if p.kind == "err" and p.stale else "sensitivity")
        else:
            out.append(names.get(op[0], op[0]))
    return out


def coarse(cls):
    return {"propagate_device": "propagate", "sensitivity_stale": "sensitivity"}.get(cls, cls)


def fast_path_ops(sysname, ops):
    """Indices of the evals the model expects on the system's fast path (a built-in cost, no co-state source on the
    segmented eval, exactly skew-Hermitian generators, order 3 or exact on the block propagators)."""
    s, m, out = system(sysname), Model(sysname), []
    for i, op in enumerate(ops):
        st = m.st
        p = m.apply(op)
        if op[0] not in ("eval", "eval_spl") or p.kind != "Jg":
            continue
        if s.fast == "segmented" and st.src is None and st.gen != "g_inexact":
            out.append(i)
        if s.fast == "blocks_prop16" and op[2] in (3, "exact"):
            out.append(i)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The runner
# ----------------------------------------------------------------------------------------------------------------------
def make_engine(sysname, monkeypatch):
    """One context in the default environment plus QOC_BLOCKS=1, configured as default_settings says."""
    from qoc_amd import GrapeEngine
    s = system(sysname)
    for k in [k for k in os.environ if k.startswith("QOC_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("QOC_BLOCKS", "1")
    A0, A = s.gens["g0"]
    e = GrapeEngine(A0, A, s.x0s["x0"][0], s.Nt, B=B)
    kind, xt, n = s.costs["trace"]
    e.set_cost_trace(xt, n)
    if s.bases:
        e.set_spline_basis(s.bases["bs"])
    return e


def _seed_bar(J, g, Jr, gr, tag):
    """blkseg_util.assert_seed's bar: |dJ| <= 1e-12, ||d dJdu|| <= 1e-10 ||dJdu||."""
    if J is not None:
        assert abs(J - Jr) <= 1e-12, (tag, "J", J, Jr, J - Jr)
    if g is not None:
        d, nr = np.linalg.norm(g - gr), np.linalg.norm(gr)
        assert d <= 1e-10 * nr, (tag, "rel dJdu", d / nr if nr else d)


def _fit(v, v0, dv):
    """v against the family v0 + t dv: (the residual's norm, t)."""
    r = (v - v0).ravel()
    d = dv.ravel()
    dd = np.vdot(d, d).real
    t = float(np.vdot(d, r).real / dd) if dd else 0.0
    return r - t * d, t


class Runner:
    def __init__(self, sysname, ops, monkeypatch, tag=""):
        self.sysname, self.ops, self.tag = sysname, list(ops), tag
        self.s = system(sysname)
        self.m = Model(sysname)
        self.e = make_engine(sysname, monkeypatch)
        self.e.set_profiling(True)
        self.lastJ = None
        self.infos = {}
        self.trace = []
        self.ncmp = 0

    # -- the engine side of one op ---------------------------------------------------------------------------------
    def _dev(self, a):
        import torch
        return torch.from_numpy(np.array(np.transpose(a, (0, 2, 1)), order="C")).cuda()  # (a writable copy)

    def _nan(self, *shape):
        import torch
        return torch.full(shape, np.nan, dtype=torch.float64, device="cuda")

    def _exec(self, op):
        e, s, name = self.e, self.s, op[0]
        nu, Nt = s.nu, s.Nt
        if name == "set_gen":
            return e.set_generators(*s.gens[op[1]])
        if name == "set_x0":
            return e.set_x0(s.x0s[op[1]][0], per_seed=s.x0s[op[1]][1])
        if name == "set_cost":
            kind, xt, n = s.costs[op[1]]
            return e.set_cost_trace(xt, n) if kind == "trace" else e.set_cost_zcalibrated(xt) if kind == "zcal" else e.set_cost_external()
        if name == "set_pen":
            return e.set_state_penalty(*[list(v) if isinstance(v, tuple) else v for v in s.pens[op[1]]])
        if name == "set_src":
            return e.set_costate_source(None if op[1] is None else s.srcs[op[1]])
        if name == "set_basis":
            return e.set_spline_basis(s.bases[op[1]])
        if name == "comm":
            return e.comm_init(1, 0, None, op[1])
        if name == "eval":
            ud, Jd, gd = self._dev(s.ctrl(op[1])), self._nan(B), self._nan(B, Nt, nu)
            self.bufs = (Jd, gd)
            e.eval_device(ud.data_ptr(), op[2], Jd.data_ptr(), gd.data_ptr())
            e.synchronize()
            return Jd.cpu().numpy(), np.transpose(gd.cpu().numpy(), (0, 2, 1))
        if name == "eval_spl":
            return e.eval_spline(s.ctrl(op[1]), op[2])
        if name == "prop":
            return e.propagate(s.ctrl(op[1]))
        if name == "prop_spl":
            return e.propagate_spline(s.ctrl(op[1]))
        if name == "prop_dev":
            ud, Jd = self._dev(s.ctrl(op[1])), self._nan(B)
            e.propagate_device(ud.data_ptr(), Jd.data_ptr())
            e.synchronize()
            return Jd.cpu().numpy()
        if name == "sens":
            return e.grape_sensitivity(s.ctrl(op[1]), op[2], lambda_final=s.lams[op[3]] if len(op) > 3 else None)
        if name == "sens_spl":
            return e.sensitivity_spline(s.ctrl(op[1]), op[2])
        if name == "sens_dev":
            ud, gd = self._dev(s.ctrl(op[1])), self._nan(B, Nt, nu)
            self.bufs = (gd,)
            try:
                e.grape_sensitivity_device(ud.data_ptr(), op[2], gd.data_ptr())
            finally:
                e.synchronize()
            return np.transpose(gd.cpu().numpy(), (0, 2, 1))
        if name in ("state", "state_dead0"):
            return e.state(op[1], seed=op[2])
        if name in ("costate", "costate_dead0"):
            return e.costate(op[1], seed=op[2])
        if name == "best":
            return e.allgather_best()
        raise KeyError(op)

    # -- one op on both sides --------------------------------------------------------------------------------------
    def _step(self, i, op):
        from qoc_amd import QOCError, StaleCacheError
        p = self.m.apply(op)
        assert p.kind != "unknown", "the model has no prediction"
        self.bufs = ()
        if p.kind == "err":
            try:
                self._exec(op)
            except QOCError as ex:
                assert type(ex) is (StaleCacheError if p.stale else QOCError) and ex.code == p.code, (type(ex), ex)
                if p.stale:
                    assert STALE_MSG in str(ex), ex
            else:
                raise AssertionError(f"no error, the model predicts code {p.code}")
            for buf in self.bufs:  # a refused device call leaves the caller's buffers as they were
                assert bool(buf.isnan().all()), "the refused call wrote its output buffer"
            return
        out = self._exec(op)
        tag = (self.sysname, self.tag, i, op)
        if p.kind == "ok":
            return
        if p.kind in ("J", "Jg", "g"):
            J, g = (out, None) if p.kind == "J" else (None, out) if p.kind == "g" else out
            if J is not None:
                self.lastJ = np.array(J)
                Jr = p.J()
                for b in range(B):
                    _seed_bar(J[b], None, Jr[b], None, tag + (b,))
            if g is not None:
                assert g.shape == p.lam_g()[1].shape, (g.shape, p.lam_g()[1].shape)
                self._grad(p, g, tag)
                info = self.e.info()
                self.infos[i] = (info["backward"], info["interp_degree"])
            return
        if p.kind == "x":
            xs = p.states()[p.seed]
            assert np.abs(out - xs[p.k]).max() <= 1e-12 * np.abs(xs).max(), (tag, np.abs(out - xs[p.k]).max())
        elif p.kind == "lam":
            lam = p.lam_g()[0][p.seed]
            d = out - lam[p.k]
            if p.zcal():  # the calibration phase is fixed to ~sqrt(eps) only (tests/test_gpu_parity.py): the family
                h = 1e-6
                dl = (p.lam_g(h)[0][p.seed][p.k] - p.lam_g(-h)[0][p.seed][p.k]) / (2 * h)
                d, t = _fit(out, lam[p.k], dl)
                assert abs(t) <= p.dtheta_bound(p.seed), (tag, "dtheta", t)
            assert np.abs(d).max() <= 1e-12 * np.abs(lam).max(), (tag, np.abs(d).max(), np.abs(lam).max())
        elif p.kind == "best":
            assert self.lastJ is not None
            assert out == (float(self.lastJ.min()), p.offset + int(np.argmin(self.lastJ))), (tag, out, self.lastJ)
            Jr = np.sort(p.J())
            if Jr[1] - Jr[0] > 1e-9:  # (no near-tie: the model's seed too)
                assert out[1] == p.offset + int(np.argmin(p.J())), (tag, out, p.J())
            return
        if p.kind in ("x", "lam") and p.zero_rows is not None:
            assert len(p.zero_rows) > 0, (tag, "no dead rows")
            assert np.all(out[p.zero_rows] == 0.0), (tag, "dead rows", out[p.zero_rows])

    def _grad(self, p, g, tag):
        gr = p.lam_g()[1]
        if not p.zcal():
            for b in range(B):
                _seed_bar(None, g[b], None, gr[b], tag + (b,))
            return
        h = 1e-6  # qoc_oracle.zcal_gradient_match's fit, with the penalty and the source in the family
        dg = (p.lam_g(h)[1] - p.lam_g(-h)[1]) / (2 * h)
        for b in range(B):
            r, t = _fit(g[b], gr[b], dg[b])
            assert np.linalg.norm(r) <= 1e-10 * np.linalg.norm(gr[b]), (tag, b, "zcal residual", np.linalg.norm(r) / np.linalg.norm(gr[b]))
            assert abs(t) <= p.dtheta_bound(b), (tag, b, "dtheta", t)

    def _route(self, op):
        """One row of the route trace: the op's name, what qoc_get_info reports of the records the op left (fwd: split
        kind, captures, the formation's degree and chain; bwd: the route) and the launches per phase since the last op."""
        info = self.e.info()
        n = self.e.phase_times(reset=True)
        return [op[0], info["backward"], info["split_forward"], int(info["fwd_captured"]), info["interp_degree"],
                info["interp_chain"]] + [n[k][1] for k in self.e.PHASES]

    def run(self):
        try:
            for i, op in enumerate(self.ops):
                try:
                    self._step(i, op)
                except Exception as ex:
                    raise AssertionError(
                        f"{self.sysname} {self.tag}: op {i} {op!r}: {type(ex).__name__}: {ex}\nthe sequence so far, as PINNED "
                        f"takes it:\n{pprint.pformat(self.ops[:i + 1], width=110)}") from ex
                self.trace.append(self._route(op))
                self.ncmp += 1
        finally:
            self.e.close()
        assert self.ncmp == len(self.ops)
        want = fast_path_ops(self.sysname, self.ops)
        if want:  # the fast paths really ran: a sequence cannot pass on fallbacks alone
            got = [self.infos[i] for i in want]
            assert any(b == self.s.fast for b, _ in got), (self.s.fast, got)
            if self.sysname == "tunable_bus":
                assert any(d > 0 for _, d in got), got
        return self


# ----------------------------------------------------------------------------------------------------------------------
# What the seed lists must cover, and the pinned sequences
# ----------------------------------------------------------------------------------------------------------------------
def required_pairs(sysname):
    """Ordered pairs of op classes (coarse: either propagate, either sensitivity) that must occur directly after one
    another, and the fine ones around a stale sensitivity."""
    pairs = [(a, b) for a in setters_of(system(sysname)) for b in FOLLOWERS]
    fine = [(a, "sensitivity_stale") for a in ("eval", "propagate_device", "propagate")]
    return pairs, fine


def missing_transitions(sysname, sequences):
    """The requirements of tests/test_gpu_call_sequences.py::test_sequences_cover_the_transitions no sequence meets."""
    s = system(sysname)
    pairs, fine = required_pairs(sysname)
    seen, seen_fine, triple, ranges = set(), set(), False, set()
    for ops in sequences:
        cls = classify(sysname, ops)
        for a, b in zip(cls, cls[1:]):
            seen.add((coarse(a), coarse(b)))
            seen_fine.add((a, b))
        triple = triple or any(coarse(a) == "eval" and coarse(b) == "propagate" and c == "costate"
                               for a, b, c in zip(cls, cls[1:], cls[2:]))
        if sysname == "tunable_bus":  # the control ranges of successive forwards
            kind = {"narrow": "n", "narrow2": "n", "cn": "n", "wide": "w", "cw": "w", "flat": "0"}
            m = Model(sysname)
            fw = "".join(kind[op[1]] for op in ops if m.apply(op).kind in ("J", "Jg"))
            ranges |= {r for r in ("nwn", "n0", "w0") if r in fw}
    miss = [p for p in pairs if p not in seen] + [p for p in fine if p not in seen_fine]
    if not triple:
        miss.append(("eval", "propagate", "costate"))
    if sysname == "tunable_bus":
        miss += [r for r in ("nwn", "n0", "w0") if r not in ranges]
    if s.fast and not all(fast_path_ops(sysname, ops) for ops in sequences):
        miss.append("a sequence without an eval on " + s.fast)
    return miss


SEEDS = {"cavity20": [2, 22, 6, 25], "zz": [7, 11, 8, 24], "tunable_bus": [6, 1, 21, 29, 16],
         "tunable_bus_cz": [5, 3, 12, 2], "cavity_dense": [7, 23, 5, 15, 6]}

_PEN_SPLIT = [("prop_dev", "narrow"), ("set_pen", "pen0"), ("sens_dev", "narrow", 3), ("sens", "narrow", "exact"),
              ("set_pen", "mu0"), ("sens", "narrow", 3), ("costate", 10, 2)]
PINNED = {
    # an external lambda_final on the dead block's rows, then a built-in cost: the dead rows exactly zero again
    "external_lambda_on_dead_rows": ("tunable_bus", [
        ("set_cost", "ext"), ("prop", "narrow"), ("sens", "narrow", 3, "lam0"), ("costate", 7, 1), ("set_cost", "trace"),
        ("prop", "narrow"), ("sens", "narrow", 3), ("costate_dead0", 7, 1), ("state_dead0", 7, 1), ("costate_dead0", 0, 2),
        ("state_dead0", 21, 0)]),
    # the interpolation coefficients recomputed, reused and recomputed on one context
    "control_range_there_and_back": ("tunable_bus", [
        ("prop", "narrow"), ("sens", "narrow", "exact"), ("eval", "wide", "exact"), ("prop", "narrow"),
        ("sens", "narrow", "exact"), ("eval", "flat", "exact")]),
    # a penalty set between the halves of the split form: the forward kept as stored / interpolating propagators
    "penalty_between_split_halves_bus": ("tunable_bus", _PEN_SPLIT),
    "penalty_between_split_halves_cz": ("tunable_bus_cz", _PEN_SPLIT),
    "state_moves_to_the_other_block": ("tunable_bus", [
        ("set_x0", "x0_odd"), ("set_cost", "trace_odd"), ("eval", "narrow", 3), ("state_dead0", 9, 0),
        ("costate_dead0", 9, 0), ("set_x0", "x0_both"), ("eval", "narrow", "exact"), ("state", 9, 0), ("costate", 9, 0)]),
    "stale_device_sensitivity_writes_nothing": ("cavity20", [
        ("eval", "u0", 3), ("sens_dev", "u0*", 3), ("costate", 14, 1), ("sens_dev", "u0", 3), ("costate", 14, 1)]),
    "block_layout_there_and_back": ("cavity20", [
        ("eval", "u0", 3), ("set_gen", "g_blk3"), ("costate", 14, 1), ("state", 14, 1), ("eval", "u1", 3),
        ("set_gen", "g0"), ("prop", "u2"), ("sens", "u2", "exact")]),
    "penalty_on_off_on_zz": ("zz", [
        ("set_pen", "pen0"), ("eval", "u0", 3), ("set_pen", "off"), ("prop", "u0"), ("sens", "u0", 3),
        ("set_pen", "pen0"), ("sens", "u0", 3), ("eval", "u0", "exact")]),
    "spline_staleness": ("zz", [
        ("prop_spl", "c0"), ("prop", "u0"), ("sens_spl", "c0", 3), ("prop_spl", "c0"), ("set_basis", "bs_half"),
        ("sens_spl", "c0", 3), ("prop_spl", "c0"), ("sens_spl", "c0", 3)]),
    "best_follows_the_last_forward": ("cavity20", [
        ("comm", 1000), ("eval", "u0", 3), ("best",), ("prop", "u3"), ("best",), ("set_cost", "trace_neg"),
        ("eval", "u0", 3), ("best",)]),
    # found by this suite (call sequences): a refused eval_spline had already overwritten the controls
    "refused_eval_spline_leaves_the_controls": ("zz", [
        ("set_cost", "ext"), ("prop", "u0"), ("eval_spl", "c0", 3), ("sens", "u0", 3, "lam0"), ("costate", 3, 1)]),
    # found by this suite: the exact gradient's 18 x 18 block exponentials on the Paterson-Stockmeyer branch (a co-state
    # source sends zz to the dense Frechet kernel; the largest amplitudes under the longer slices) read a never
    # written LDS pad column: NaN in single slices of dJdu, whenever a kernel before had left one there
    "exact_gradient_on_large_norm_blocks_of_18": ("zz", [
        ("set_gen", "g_dt"), ("set_cost", "zcal"), ("set_src", "src0"), ("set_pen", "pen0"), ("set_x0", "x0_seed"),
        ("eval", "u3", 1), ("sens", "u3", 1), ("eval", "u2", "exact"), ("eval", "u1", "exact"), ("sens", "u1", "exact")]),
    # found by this suite: a propagate zeroed the newly dead rows of the co-states the last sensitivity left
    "old_costates_survive_a_propagate_on_another_block": ("tunable_bus", [
        ("eval", "narrow", 3), ("set_x0", "x0_odd"), ("set_cost", "trace_odd"), ("prop", "narrow"), ("costate", 7, 1),
        ("sens", "narrow", 3), ("costate_dead0", 7, 1)]),
}


# ----------------------------------------------------------------------------------------------------------------------
# The pinned sequences' route trace
# ----------------------------------------------------------------------------------------------------------------------
ROUTES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_sequence_routes.json")


def pinned_routes():
    """tests/golden/call_sequence_routes.json: per PINNED sequence, per op, Runner._route's row.  A pull request that
    changes a route on purpose regenerates the file on an MI355X, from the repository's root after a build:

        python tests/engine_model.py

    and shows the rows that moved in its diff."""
    import json
    with open(ROUTES) as f:
        return json.load(f)


class _Environ:
    """monkeypatch's two calls, for a run outside pytest."""
    delenv = staticmethod(os.environ.__delitem__)
    setenv = staticmethod(os.environ.__setitem__)


if __name__ == "__main__":
    import json
    import torch
    torch.empty(1, device="cuda")  # torch's HIP runtime first, as tests/conftest.py built_lib
    out = sys.argv[1] if len(sys.argv) > 1 else ROUTES
    traces = {name: Runner(sysname, ops, _Environ, tag=name).run().trace for name, (sysname, ops) in PINNED.items()}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": [\n  ' + ",\n  ".join(json.dumps(row) for row in rows) + "]"
                                   for name, rows in traces.items()) + "\n}\n")
    print("wrote", out)
