"""qoc_eval_envelope: J and dJ/dp of the continuous-envelope run, the discrete adjoint of fixed-step Tsit5, against the
numpy adjoint of tests/envgrad_util.py (pinned on the CPU by tests/test_envelope_grad_algebra.py).

Bar, per seed: |dJ| <= 1e-12 and ||dg|| / ||g|| <= 1e-10 (the project's fp64 parity bar).  Under the z-calibrated cost
the golden-section search fixes the calibration phase only to ~sqrt(eps) and lambda_N carries it linearly, so the
gradient is held to the oracle's family in that phase (qoc_oracle.zcal_gradient_match's construction: residual
<= 1e-10, the phase within qoc_oracle.zcal_dtheta_bound), as tests/test_gpu_parity.py::test_zcalibrated_cost does.
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import envgrad_util as E
import qoc_oracle as O

pytestmark = pytest.mark.gpu


def _bar(tag, J, Jr, g, gr):
    dJ = None if J is None else abs(J - Jr)
    dg = np.linalg.norm(g - gr) / np.linalg.norm(gr)
    print(f"{tag}: |dJ| = {dJ}, rel |dg| = {dg:.3e}, |g| = {np.linalg.norm(gr):.3e}")
    if J is not None:
        assert dJ <= 1e-12, (tag, J, Jr)
    assert dg <= 1e-10, (tag, g, gr)


def _engine(A0, A, x0, B, per_seed=False, precision="fp64"):
    from qoc_amd import GrapeEngine
    e = GrapeEngine(A0, A, x0[0] if per_seed else x0, 1, B=B, precision=precision)
    if per_seed:
        e.set_x0(x0, per_seed=True)
    return e


def _mark(e, seed=0):
    """An ordinary propagate whose states a refused call must leave readable and current."""
    u = np.random.default_rng(seed).uniform(-0.05, 0.05, (e.B, e.nu, e.Nt))
    J = e.propagate(u)
    return u, J, np.stack([e.state(-1, seed=b) for b in range(e.B)])


def _unchanged(e, mark):
    u, J, x = mark
    assert np.array_equal(np.stack([e.state(-1, seed=b) for b in range(e.B)]), x)
    lam = np.zeros((e.B, e.N, e.m), dtype=complex) if e.cost_kind == "external" else None
    e.grape_sensitivity(u, 3, lambda_final=lam)  # not stale: the refused call began no forward


# ---- parity on the reference's systems ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["drag", "sinebasis"])
def test_transmon_trace_matches_numpy_adjoint(built_lib, kind):
    """The two parameter rows of test_gpu_ode.py::test_envelope_drag_sinebasis_match_oracle, dt = 0.05, m = 2."""
    A0, A = E.transmon()
    x0 = np.eye(4, dtype=complex)[:, :2]
    xt = np.eye(4, dtype=complex)[:, [1, 0]]
    if kind == "drag":
        P = np.array([[20.0, 5.0, 0.16, 0.4], [24.0, 4.0, 0.13, -0.2]])
    else:
        P = np.array([[20.0, 0.05, 0.01, -0.02, 0.03, 0.004, 0.0], [20.0, 0.07, -0.01, 0.01, 0.0, -0.01, 0.02]])
    e = _engine(A0, A, x0, 2)
    e.set_cost_trace(xt, 2)
    Jf, dJ = E.trace_cost(xt, 2)
    for tg in sorted(set(P[:, 0])):  # one gate time per call (tgate is shared by the batch)
        J, g, x = e.eval_envelope(kind, P, float(tg), 0.05)
        Jp, xp = e.propagate_envelope(kind, P, float(tg), 0.05)
        assert np.array_equal(J, Jp) and np.array_equal(x, xp)  # the forward's J and x(tgate), bit for bit
        for b in np.nonzero(P[:, 0] == tg)[0]:
            xr, gr = E.adjoint(A0, A, kind, P[b], x0, float(tg), 0.05, dJ)
            assert np.abs(x[b] - xr).max() < 1e-12
            _bar(f"{kind} seed {b}", J[b], Jf(xr), g[b], gr)
    e.close()


def test_tunable_bus_matches_numpy_adjoint(built_lib):
    """N = 27, m = 1, 1750 steps at |H| ~ 104 rad/ns: three rows around the reference's pulse."""
    A0, A, x0, xt, w = E.tunable_bus_setup()
    P = np.array([[2.0, 1.5, 0.25, w, 0.13], [1.8, 1.7, 0.22, w * 1.01, 0.15], [2.2, 1.2, 0.27, w * 0.99, 0.10]])
    e = _engine(A0, A, x0, 3)
    e.set_cost_trace(xt, 1)
    Jf, dJ = E.trace_cost(xt, 1)
    J, g, x = e.eval_envelope("tunable_bus", P, 3.5, 2e-3)
    Jp, _ = e.propagate_envelope("tunable_bus", P, 3.5, 2e-3)
    assert np.array_equal(J, Jp)
    for b in range(3):
        xr, gr = E.adjoint(A0, A, "tunable_bus", P[b], x0, 3.5, 2e-3, dJ)
        _bar(f"tunable_bus seed {b}", J[b], Jf(xr), g[b], gr)
    e.close()


def _transmon4():
    A0, A = E.transmon()
    rng = np.random.default_rng(11)
    x0, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    xt, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    return A0, A, x0, xt


def test_zcal_matches_oracle_family(built_lib):
    """m = 4 on the transmon.  lambda_N of the numpy adjoint comes from the oracle's closure at its own calibration
    phase plus a fitted shift (see the module docstring).  Measured on an MI355X: residual 1.1e-16 / 2.1e-16 at shifts
    of 1.7e-9 / -3.1e-8 (bound 2.6e-7); without the fit the two sides differ by 2.4e-9 / 4.9e-8, the phase's doing."""
    A0, A, x0, xt = _transmon4()
    P = np.array([[20.0, 5.0, 0.16, 0.4], [20.0, 4.0, 0.13, -0.2]])
    e = _engine(A0, A, x0, 2)
    e.set_cost_zcalibrated(xt)
    J, g, x = e.eval_envelope("drag", P, 20.0, 0.05)
    assert J is not None
    for b in range(2):
        def grad(dth):
            return E.adjoint(A0, A, "drag", P[b], x0, 20.0, 0.05, O.setup_infidelity_zcalibrated_shifted(xt, dth)[1])
        (xr, g0), h = grad(0.0), 1e-6
        d = (grad(h)[1] - grad(-h)[1]) / (2 * h)
        r = g[b] - g0
        t = float(np.dot(d, r) / np.dot(d, d))
        res = np.linalg.norm(r - t * d) / np.linalg.norm(g0)
        bound = O.zcal_dtheta_bound(xt, xr)
        Jr = O.setup_infidelity_zcalibrated(xt)[0](xr)
        print(f"zcal seed {b}: |dJ| = {abs(J[b] - Jr)}, residual = {res:.3e}, dtheta = {t:.3e} (bound {bound:.3e}), "
              f"plain rel |dg| = {np.linalg.norm(r) / np.linalg.norm(g0):.3e}")
        assert abs(J[b] - Jr) <= 1e-12
        assert res <= 1e-10 and abs(t) <= bound
    e.close()


def test_external_cost_takes_lambda_final(built_lib):
    from qoc_amd import QOCError
    A0, A, x0, _ = _transmon4()
    rng = np.random.default_rng(5)
    lam = rng.standard_normal((2, 4, 4)) + 1j * rng.standard_normal((2, 4, 4))
    P = np.array([[20.0, 0.05, 0.01, -0.02, 0.03], [20.0, 0.07, -0.01, 0.01, 0.0]])
    e = _engine(A0, A, x0, 2)
    e.set_cost_external()
    J, g, x = e.eval_envelope("sinebasis", P, 20.0, 0.05, lambda_final=lam)
    assert J is None
    for b in range(2):
        xr, gr = E.adjoint(A0, A, "sinebasis", P[b], x0, 20.0, 0.05, lambda xN: lam[b])
        assert np.abs(x[b] - xr).max() < 1e-12
        _bar(f"external seed {b}", None, None, g[b], gr)
    mark = _mark(e)
    with pytest.raises(QOCError) as ei:  # missing lambda_final
        e.eval_envelope("sinebasis", P, 20.0, 0.05)
    assert ei.value.code == -1
    import torch
    d = torch.zeros(2, 5, dtype=torch.float64, device="cuda")
    with pytest.raises(QOCError) as ei:  # the device form has no lambda_final
        e.eval_envelope_device("sinebasis", d.data_ptr(), 5, 20.0, 0.05, 0, d.data_ptr())
    assert ei.value.code == -1
    _unchanged(e, mark)
    e.close()


# ---- the smallest shapes that can go wrong -------------------------------------------------------------------------
def _random_system(N, nu, seed, gamma=0.0):
    """Random skew-Hermitian generators of 2-norm <= 1; gamma > 0 adds -gamma diag(0..1) to A0: not skew-Hermitian."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nu + 1):
        H = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        H = (H + H.conj().T) / 2
        out.append(-1j * H / np.linalg.norm(H, 2))
    if gamma:
        out[0] = out[0] - gamma * np.diag(np.linspace(0.0, 1.0, N))
    return out[0], out[1:]


def _random_states(N, m, B, seed):
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((B, N, m)) + 1j * rng.standard_normal((B, N, m))
    x0 /= np.linalg.norm(x0, axis=(1, 2), keepdims=True)
    xt = rng.standard_normal((N, m)) + 1j * rng.standard_normal((N, m))
    return x0, xt / np.linalg.norm(xt)


def _params(kind, B, seed, npar=None):
    rng = np.random.default_rng(seed)
    if kind == "tunable_bus":  # theta / pi stays within 0.25 +- 0.15: away from cos(theta) = 0
        return np.column_stack([rng.uniform(1.5, 2.5, B), rng.uniform(1.0, 2.0, B), rng.uniform(0.2, 0.3, B),
                                rng.uniform(3.0, 5.0, B), rng.uniform(0.05, 0.15, B)])
    if kind == "drag":
        return np.column_stack([rng.uniform(3.0, 5.0, B), rng.uniform(0.8, 1.5, B), rng.uniform(0.3, 1.0, B),
                                rng.uniform(-1.0, 1.0, B)])
    return np.column_stack([rng.uniform(3.0, 5.0, B), rng.uniform(-0.5, 0.5, (B, npar - 1)) / np.sqrt(npar)])


def _shape_case(monkeypatch, N, m, kind, nsteps, ckpt, gamma=0.0, npar=7, B=3, dt=0.05, reference=True, ws_mb=None):
    """ckpt: the forced spacing, or None: chosen by the engine from the workspace budget (ws_mb MiB, or its own)."""
    for var, val in (("QOC_ENV_CKPT", ckpt), ("QOC_ENV_WS_MB", ws_mb)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    nu = 1 if kind == "tunable_bus" else 2
    A0, A = _random_system(N, nu, 100 + N, gamma)
    x0, xt = _random_states(N, m, B, 200 + N + m)
    P = _params(kind, B, 300 + N, npar)
    e = _engine(A0, A, x0, B, per_seed=True)
    e.set_cost_trace(xt, 1)
    tg = nsteps * dt
    J, g, x = e.eval_envelope(kind, P, tg, dt)
    Jp, xp = e.propagate_envelope(kind, P, tg, dt)
    e.close()
    assert np.array_equal(J, Jp) and np.array_equal(x, xp)
    if reference:
        Jf, dJ = E.trace_cost(xt, 1)
        for b in range(B):
            xr, gr = E.adjoint(A0, A, kind, P[b], x0[b], tg, dt, dJ)
            _bar(f"N={N} m={m} {kind} steps={nsteps} C={ckpt} seed {b}", J[b], Jf(xr), g[b], gr)
    return g


@pytest.mark.parametrize("N,m,kind,gamma,npar", [
    (2, 1, "drag", 0.0, 4),
    (2, 5, "sinebasis", 0.0, 7),          # 5 columns on 4 waves: a wave loops
    (27, 2, "drag", 0.3, 4),              # A0 not skew-Hermitian: A^H is not -A
    (27, 5, "tunable_bus", 0.0, 5),
    (27, 1, "sinebasis", 0.0, 63),        # the last lane of the parameter cap
    # the largest fp64 size the envelope path admits (a context of N > 48 runs the large-N pipeline, which
    # qoc_propagate_envelope refuses too: test_refusals_change_nothing): two generator copies do not fit beside the
    # ring, A^H is read in place
    (48, 1, "tunable_bus", 0.2, 5),
    (48, 2, "drag", 0.0, 4),
])
def test_shapes_match_numpy_adjoint(built_lib, monkeypatch, N, m, kind, gamma, npar):
    _shape_case(monkeypatch, N, m, kind, 23, 7, gamma=gamma, npar=npar)


@pytest.mark.parametrize("nsteps", [1, 5, 64, 65])
def test_checkpoint_spacings_agree_bitwise(built_lib, monkeypatch, nsteps):
    """Segment tails, a single short segment, exactly one full segment: C in {1, 7, 64} give the same bits, and those
    match the numpy adjoint (N = 5, m = 5: a wave loops over two columns)."""
    gs = [_shape_case(monkeypatch, 5, 5, "drag", nsteps, C, gamma=0.1, reference=C == 7) for C in (1, 7, 64)]
    assert np.array_equal(gs[0], gs[1]) and np.array_equal(gs[0], gs[2])


@pytest.mark.parametrize("N,m,kind", [(27, 5, "sinebasis"), (48, 4, "drag")])
def test_checkpoint_spacings_agree_bitwise_large(built_lib, monkeypatch, N, m, kind):
    """The same with A^H read in place, and with the LDS ring bounding a forced spacing (N = 48, nu = 2, four column
    waves: 16 steps)."""
    gs = [_shape_case(monkeypatch, N, m, kind, 65, C, reference=False) for C in (1, 7, 64)]
    assert np.array_equal(gs[0], gs[1]) and np.array_equal(gs[0], gs[2])


def test_spacing_chosen_from_the_workspace_budget(built_lib, monkeypatch):
    """No forced spacing: a checkpoint of B = 3, m = 5, N = 5 takes 2400 bytes, so a budget of 0.01 MiB holds four and
    65 steps run at C = 17; the bits are those of C = 1 (the default budget).  A budget that needs a spacing beyond the
    LDS ring (2000 steps on one checkpoint; the ring holds 498) is refused with nothing changed."""
    from qoc_amd import QOCError
    g1 = _shape_case(monkeypatch, 5, 5, "drag", 65, None, gamma=0.1, reference=False)
    g17 = _shape_case(monkeypatch, 5, 5, "drag", 65, None, gamma=0.1, reference=False, ws_mb=0.01)
    gf = _shape_case(monkeypatch, 5, 5, "drag", 65, 17, gamma=0.1, reference=False)
    assert np.array_equal(g1, g17) and np.array_equal(g1, gf)
    monkeypatch.delenv("QOC_ENV_CKPT", raising=False)
    monkeypatch.setenv("QOC_ENV_WS_MB", "0.001")
    A0, A = _random_system(5, 2, 105, 0.1)
    x0, xt = _random_states(5, 5, 3, 210)
    e = _engine(A0, A, x0, 3, per_seed=True)
    e.set_cost_trace(xt, 1)
    mark = _mark(e)
    with pytest.raises(QOCError) as ei:
        e.eval_envelope("drag", _params("drag", 3, 305), 100.0, 0.05)
    assert ei.value.code == -5 and "spacing" in str(ei.value)
    _unchanged(e, mark)
    e.close()


def test_repeatable_and_device_form_bitwise(built_lib):
    import torch
    A0, A = _random_system(9, 2, 7)
    x0, xt = _random_states(9, 3, 3, 8)
    P = _params("drag", 3, 9)
    e = _engine(A0, A, x0, 3, per_seed=True)
    e.set_cost_trace(xt, 1)
    J1, g1, _ = e.eval_envelope("drag", P, 2.0, 0.05)
    J2, g2, _ = e.eval_envelope("drag", P, 2.0, 0.05)
    assert np.array_equal(J1, J2) and np.array_equal(g1, g2)
    dev = torch.device("cuda", e.device)
    dP = torch.from_numpy(P).to(dev)
    dJ = torch.zeros(3, dtype=torch.float64, device=dev)
    dg = torch.zeros(3, 4, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    e.eval_envelope_device("drag", dP.data_ptr(), 4, 2.0, 0.05, dJ.data_ptr(), dg.data_ptr())
    e.synchronize()
    assert np.array_equal(dJ.cpu().numpy(), J1) and np.array_equal(dg.cpu().numpy(), g1)
    e.close()


# ---- what the call leaves on the context ---------------------------------------------------------------------------
def _all(e, f):
    return np.stack([np.stack([f(k, seed=b) for k in range(e.Nt + 1)]) for b in range(e.B)])


def test_context_is_left_as_after_propagate_envelope(built_lib):
    from qoc_amd import QOCError, systems
    prob = systems.cavity_problem(N_cavity=6, Nt=12)
    u = systems.cavity_controls(2, prob.Nt, seed=3)
    P = np.array([[3.0, 0.05, 0.01, -0.02, 0.03], [3.0, 0.07, -0.01, 0.01, 0.0]])
    got = []
    for use_eval in (True, False):
        from qoc_amd import GrapeEngine
        e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=2)
        e.set_cost_trace(prob.x_target, prob.n)
        e.propagate(u)
        e.grape_sensitivity(u, 3)
        lam = _all(e, e.costate)
        if use_eval:
            J, g, x = e.eval_envelope("sinebasis", P, 3.0, 0.1)
        else:
            J, x = e.propagate_envelope("sinebasis", P, 3.0, 0.1)
        rec = {"J": J, "x": x, "info": e.info(), "lam": _all(e, e.costate)}
        assert np.array_equal(rec["lam"], lam)  # the co-states of the last grape_sensitivity, untouched
        try:
            rec["state"] = e.state(-1, seed=1)
        except QOCError as ex:
            rec["state"] = ex.code
        try:
            e.grape_sensitivity(u, 3)
            rec["sens"] = "ok"
        except QOCError as ex:
            rec["sens"] = ex.code
        rec["J2"] = e.propagate(u)
        rec["g2"] = e.grape_sensitivity(u, 3)
        rec["info2"] = e.info()
        got.append(rec)
        e.close()
    a, b = got
    assert np.array_equal(a["J"], b["J"]) and np.array_equal(a["x"], b["x"])
    assert a["info"] == b["info"] and a["info2"] == b["info2"]
    assert np.array_equal(a["state"], b["state"]) and a["sens"] == b["sens"]
    assert np.array_equal(a["J2"], b["J2"]) and np.array_equal(a["g2"], b["g2"])


def test_refusals_change_nothing(built_lib):
    from qoc_amd import QOCError
    A0, A = E.transmon()
    x0 = np.eye(4, dtype=complex)[:, :2]
    xt = np.eye(4, dtype=complex)[:, [1, 0]]
    P = np.array([[20.0, 5.0, 0.16, 0.4]])

    def refused(e, code, *args, **kw):
        with pytest.raises(QOCError) as ei:
            e.eval_envelope(*args, **kw)
        assert ei.value.code == code, str(ei.value)
        return str(ei.value)

    e = _engine(A0, A, x0, 1)
    e.set_cost_trace(xt, 2)
    mark = _mark(e)
    refused(e, -1, "tunable_bus", np.array([[2.0, 1.5, 0.25, 4.0, 0.13]]), 3.5, 0.1)  # drives one control, nu = 2
    refused(e, -1, "drag", np.zeros((1, 65)), 20.0, 0.1)                               # np out of range
    refused(e, -1, "drag", P, 20.0, 0.0)
    _unchanged(e, mark)
    e.close()

    # N = 64 in fp64 is a large-N context: refused like qoc_propagate_envelope, with the same message
    A64, Aj64 = _random_system(64, 1, 1)
    x64, xt64 = _random_states(64, 1, 1, 2)
    e = _engine(A64, Aj64, x64[0], 1)
    e.set_cost_trace(xt64, 1)
    mark = _mark(e)
    P64 = _params("tunable_bus", 1, 3)
    msg = refused(e, -5, "tunable_bus", P64, 1.0, 0.05)
    with pytest.raises(QOCError) as ei:
        e.propagate_envelope("tunable_bus", P64, 1.0, 0.05)
    assert ei.value.code == -5 and str(ei.value) == msg
    _unchanged(e, mark)
    e.close()

    e = _engine(A0, A, x0, 1, precision="fp32")
    e.set_cost_trace(xt, 2)
    mark = _mark(e)
    assert "fp64" in refused(e, -5, "drag", P, 20.0, 0.1)
    _unchanged(e, mark)
    e.close()

    # two parity sectors (even / odd rows) that the generators keep apart: compress_states applies
    N, rng = 6, np.random.default_rng(3)
    r1, r2 = list(range(0, N, 2)), list(range(1, N, 2))

    def block_gen():
        H = np.zeros((N, N), complex)
        for r in (r1, r2):
            G = rng.standard_normal((3, 3)) + 1j * rng.standard_normal((3, 3))
            H[np.ix_(r, r)] = (G + G.conj().T) / 2
        return -1j * H / np.linalg.norm(H, 2)
    x0b, xtb = np.zeros((N, 2), complex), np.zeros((N, 2), complex)
    x0b[r1[0], 0] = x0b[r2[0], 1] = xtb[r1[1], 0] = xtb[r2[1], 1] = 1.0
    e = _engine(block_gen(), [block_gen(), block_gen()], x0b, 1)
    e.set_cost_trace(xtb, 2)
    Pb = np.array([[3.0, 1.0, 0.5, 0.4]])
    e.set_compression(((r1, [0]), (r2, [1])))
    mark = _mark(e)
    assert "compression" in refused(e, -5, "drag", Pb, 3.0, 0.1)
    _unchanged(e, mark)
    e.set_compression(None)
    J, g, x = e.eval_envelope("drag", Pb, 3.0, 0.1)
    assert np.all(np.isfinite(g)) and np.linalg.norm(g) > 0
    e.close()


# ---- calibration end to end ------------------------------------------------------------------------------------------
def test_drag_calibration_reaches_the_reference_optimum(built_lib):
    """DRAG on the transmon, tgate = 20, sigma = 5, dt = 0.1, free (A, xi) in [0, 1] x [-3, 3]: with the numpy adjoint
    and scipy's L-BFGS-B all four starts reach J* = 0.0992123093 at (0.345148, 2.21530) (scatter 9e-13 in J, 2e-6 in
    xi); minimize_batched stops by its own rule, hence the margins 1e-8 and 1e-4."""
    import torch
    from qoc_amd.optimize import minimize_batched
    A0, A = E.transmon()
    x0 = np.eye(4, dtype=complex)[:, :2]
    xt = np.eye(4, dtype=complex)[:, [1, 0]]
    e = _engine(A0, A, x0, 4)
    e.set_cost_trace(xt, 2)

    def full(v):
        return np.column_stack([np.full(4, 20.0), np.full(4, 5.0), v])

    def fg(c):
        J, g, _ = e.eval_envelope("drag", full(c.numpy()), 20.0, 0.1)
        return torch.from_numpy(J.copy()), torch.from_numpy(g[:, 2:4].copy())

    c0 = torch.tensor([[0.16, 0.4], [0.3, 0.0], [0.2, -0.5], [0.35, 1.0]], dtype=torch.float64)
    res = minimize_batched(fg, c0, lower=torch.tensor([0.0, -3.0], dtype=torch.float64),
                           upper=torch.tensor([1.0, 3.0], dtype=torch.float64), max_iter=60)
    v, J = res.c.numpy(), res.f.numpy()
    print("calibration: evals", res.n_evals, "J", J, "v", v)
    Jg, g, _ = e.eval_envelope("drag", full(v), 20.0, 0.1)
    Jf, dJ = E.trace_cost(xt, 2)
    for b in range(4):
        assert abs(J[b] - 0.0992123093) <= 1e-8, (b, J[b])
        assert abs(v[b, 0] - 0.345148) <= 1e-4 and abs(v[b, 1] - 2.21530) <= 1e-4, (b, v[b])
    xr, gr = E.adjoint(A0, A, "drag", full(v)[0], x0, 20.0, 0.1, dJ)
    dJ0 = abs(Jg[0] - Jf(xr))
    print("final point: |dJ| =", dJ0, "g =", g[0], "numpy g =", gr)
    assert dJ0 <= 1e-12
    # at the optimum the free components vanish: the bar applies to the whole gradient (tgate and sigma included)
    assert np.linalg.norm(g[0] - gr) / np.linalg.norm(gr) <= 1e-10
    e.close()
