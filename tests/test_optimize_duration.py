"""CPU: the duration form of the device optimiser at its boundary (include/qoc.h qoc_opt_create_duration) and the host
constraints of z = [c, τ] (qoc_amd.optimize.SplineGrapeDuration.cons).  No GPU compute call is made."""
import ctypes as C

import numpy as np
import pytest
import torch

NS, NU, B = 6, 2, 4
NC = NS * NU


def _create(lib, n=NC + 1, ns=NS, nu=NU, memory=10, tau=(0.5, 2.0), kappa=0.05):
    from qoc_amd import _lib as L
    p = L.OptParams(n=n, ns=ns, nu=nu, lower=-0.4, upper=0.4, g_upper=(C.c_double * 2)(2.0, 1.0), max_iter=5,
                    memory=memory, outer_iters=2, max_ls=12, rho0=10.0, gtol=1e-9, order=3)
    d = L.OptDuration(tau_lower=tau[0], tau_upper=tau[1], time_weight=kappa)
    h = C.c_void_p()
    rc = lib.qoc_opt_create_duration(C.byref(h), 0, 3, C.byref(p), C.byref(d))
    return rc, h, lib.qoc_last_error(None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(tau=(0.0, 2.0)), -1, b"tau_lower"),
    (dict(tau=(-1.0, 2.0)), -1, b"tau_lower"),
    (dict(tau=(float("nan"), 2.0)), -1, b"tau_lower"),
    (dict(tau=(float("inf"), float("inf"))), -1, b"tau_lower"),
    (dict(tau=(2.0, 0.5)), -1, b"tau_lower"),
    (dict(tau=(0.5, float("nan"))), -1, b"tau_lower"),
    (dict(kappa=float("inf")), -1, b"time_weight"),
    (dict(kappa=float("nan")), -1, b"time_weight"),
    (dict(n=NC), -1, b"ns * nu + 1"),       # the plain form's n
    (dict(n=NC + 2), -1, b"ns * nu + 1"),
    (dict(n=257, ns=0, nu=0), -5, b"n <= 256"),
    (dict(n=257, ns=128, nu=2), -5, b"n <= 256"),
    (dict(memory=17), -5, b"memory <= 16"),
    (dict(n=0, ns=0, nu=0), -1, b"invalid optimiser dimensions"),
])
def test_create_duration_rejects_bad_arguments_before_touching_the_gpu(built_lib, kw, code, text):
    """This machine has no GPU: a call that reached hipSetDevice would return QOC_ERR_HIP (-2), not these codes."""
    rc, h, msg = _create(built_lib, **kw)
    assert rc == code and not h.value, (rc, msg)
    assert text in msg


def test_create_duration_null_arguments(built_lib):
    from qoc_amd import _lib as L
    h = C.c_void_p()
    p = L.OptParams(n=3, memory=4, max_ls=2)
    assert built_lib.qoc_opt_create_duration(C.byref(h), 0, 2, C.byref(p), None) == -1 and not h.value
    assert built_lib.qoc_opt_create_duration(C.byref(h), 0, 2, None, C.byref(L.OptDuration(0.5, 2.0, 0.0))) == -1


def _z():
    rng = np.random.default_rng(5)
    return torch.from_numpy(np.concatenate([rng.uniform(-0.4, 0.4, size=(B, NC)), rng.uniform(0.8, 1.6, size=(B, 1))], 1))


class _StubEngine:
    """What SplineGrapeDuration's constructor and its host route of cons touch."""
    ns, nu, B = NS, NU, B

    def set_spline_basis(self, Bs):
        pass


def test_duration_constraints_on_a_host_z():
    from qoc_amd.optimize import SplineGrapeDuration, duration_constraints_torch, spline_constraints_torch
    z = _z()
    c = z[:, :NC].contiguous()
    g_ref, j_ref = spline_constraints_torch(c, NS, NU)
    obj = SplineGrapeDuration(_StubEngine(), None, time_weight=0.05)
    for g, gj in (obj.cons(z), obj.cons(z.numpy()), duration_constraints_torch(z, NS, NU)):
        assert g.shape == (B, 2) and gj.shape == (B, 2, NC + 1)
        assert torch.equal(g, g_ref) and torch.equal(gj[:, :, :NC], j_ref)
        assert torch.equal(gj[:, :, NC], torch.zeros(B, 2, dtype=torch.float64))
    # τ does not enter: another τ, the same values
    z2 = z.clone()
    z2[:, NC] *= 3.0
    assert torch.equal(obj.cons(z2)[0], g_ref)

    # central differences, h = 1e-5.  The bar is what spline_constraints_torch's own Jacobian achieves against the same
    # differences on the same c (measured on the CPU: max |fd - jac| = 7.5e-11 at h = 1e-5, 7.3e-9 at 1e-4, 1.1e-10 at
    # 1e-6): the c columns are that Jacobian, so they may not do worse; the τ column's difference is exactly zero.
    h = 1e-5
    gj = obj.cons(z)[1]
    fd = torch.zeros(B, 2, NC + 1, dtype=torch.float64)
    fd_ref = torch.zeros(B, 2, NC, dtype=torch.float64)
    for i in range(NC + 1):
        e = torch.zeros_like(z)
        e[:, i] = h
        fd[:, :, i] = (obj.cons(z + e)[0] - obj.cons(z - e)[0]) / (2 * h)
        if i < NC:
            fd_ref[:, :, i] = (spline_constraints_torch(c + e[:, :NC], NS, NU)[0]
                               - spline_constraints_torch(c - e[:, :NC], NS, NU)[0]) / (2 * h)
    bar = float((fd_ref - j_ref).abs().max())
    err = float((fd[:, :, :NC] - gj[:, :, :NC]).abs().max())
    print(f"fd error of the c columns {err:.3e}, of spline_constraints_torch's own Jacobian {bar:.3e}")
    assert bar <= 1e-9  # the differences themselves are sound
    assert err <= bar
    assert torch.equal(fd[:, :, NC], torch.zeros(B, 2, dtype=torch.float64))


def test_host_machine_takes_the_duration_constraints():
    """minimize_ticks with vector bounds and cons = duration_constraints_torch on an analytic objective: the τ entry
    obeys its own bounds, the c part the scalar ones, and the norm constraint binds on c alone."""
    from qoc_amd.optimize import duration_constraints_torch, minimize_ticks
    t = torch.cat([torch.full((NC,), 0.3, dtype=torch.float64), torch.tensor([5.0], dtype=torch.float64)])

    def fg(z):
        return 0.5 * ((z - t) ** 2).sum(1), z - t
    lo = np.concatenate([np.full(NC, -0.4), [0.5]])
    hi = np.concatenate([np.full(NC, 0.4), [2.0]])
    res = minimize_ticks(fg, torch.zeros(2, NC + 1, dtype=torch.float64), lower=lo, upper=hi,
                         cons=lambda z: duration_constraints_torch(z, NS, NU), g_upper=[0.5, 1.0], max_iter=40,
                         outer_iters=4, gtol=1e-8)
    z = res.c.numpy()
    assert (z[:, NC] == 2.0).all()                        # its own upper bound, far above the scalar 0.4
    assert abs(np.linalg.norm(z[0, :NC]) - 0.5) <= 1e-3   # ||c|| <= 0.5 binds (0.3 sqrt(12) > 0.5); τ = 2 is not in it
    assert float(res.lam[:, 0].min()) > 0
