"""GPU: the three spline kernels (csrc/qoc_spline.hpp) alone, at the sizes where their loops take another pass.

k_spline_u and k_spline_grad are launched with at most 4096 blocks of 256 threads and stride over the rest; the
stride loops iterate only past B Nt nu = 1 048 576 elements (k_spline_u) or B ns nu = 16 384 outputs, one wave each
(k_spline_grad).  k_spline_constraints strides over nc with 256 threads and has two zero-norm branches.

Spline map and transpose: eval_spline / eval_spline_device with c against eval_device with u = Bs c built in numpy
(|dJ| <= 1e-12; dJdc against Bs' dJdu at relative 1e-10, every seed: the project's fp64 bars) and three seeds
against the oracle.  Before every checked call the engine evaluates other coefficients, so an element a kernel fails
to write holds another problem's value, not this one's.

Constraints: against a numpy.longdouble evaluation, at the summation bound: norms relative nc eps; Jacobian entries
relative (nc + 4) eps plus the floor eps max|c| / g (the two rounded differences of an entry that cancels); exact
zeros with ==.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import blkseg_util
import qoc_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)

SPLINE_CASES = {
    # B Nt nu = 1 064 960 > 4096 * 256: seeds 2017.. are written by the second pass of k_spline_u
    "zz_B2048_Nt260_ns4": dict(system="zz", B=2048, Nt=260, ns=4),
    # B ns nu = 20 480 outputs > 16 384 waves: seeds 820.. are summed by the second pass of k_spline_grad
    "zz_B1024_Nt20_ns10": dict(system="zz", B=1024, Nt=20, ns=10),
    "zz_B3_Nt20_ns1": dict(system="zz", B=3, Nt=20, ns=1),
    "blocks_nu1_B2_Nt70_ns5": dict(system="blocks", B=2, Nt=70, ns=5),
}


def _c3(c, ns, nu):
    """(B, nc) in the device layout (s + ns j) -> eval_spline's (B, ns, nu)."""
    return c.reshape(c.shape[0], nu, ns).transpose(0, 2, 1)


@pytest.mark.parametrize("name", list(SPLINE_CASES))
def test_spline_map_and_transpose_shapes(built_lib, name):
    """k_spline_u's and k_spline_grad's grid-stride loops on their second pass (B = 2048, Nt = 260; B = 1024,
    ns = 10), ns = 1 and nu = 1.  Measured on the MI355X over the four cases: max |J - J(u)| 3.4e-16, max rel dJdc
    against Bs' dJdu 2.1e-14; against the oracle max |dJ| 1.9e-15, rel dJdc 3.3e-14."""
    from qoc_amd import GrapeEngine, systems
    spec = SPLINE_CASES[name]
    B, Nt, ns = spec["B"], spec["Nt"], spec["ns"]
    if spec["system"] == "zz":
        prob = systems.zz_problem(Nt)
    else:
        prob = blkseg_util.block_problem(2, 7, 1, 3, Nt=Nt, seed=21)[0]
    nu = len(prob.A)
    nc = ns * nu
    Bs = systems.spline_matrix(10.0, Nt, ns)
    rng = np.random.default_rng(5)
    c = 0.2 * rng.standard_normal((B, nc))
    other = 0.2 * rng.standard_normal((B, nc))
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_cost_trace(prob.x_target, prob.n)
    e.set_spline_basis(Bs)
    # host form
    e.eval_spline(_c3(other, ns, nu))
    J, g = e.eval_spline(_c3(c, ns, nu))  # g: (B, ns, nu)
    # device form, outputs NaN until written
    od, cd = torch.from_numpy(other).to(DEV), torch.from_numpy(c).to(DEV)
    Jd = torch.full((B,), np.nan, dtype=torch.float64, device=DEV)
    gd = torch.full((B, nc), np.nan, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    e.eval_spline_device(od.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    Jd.fill_(np.nan)
    gd.fill_(np.nan)
    torch.cuda.synchronize()
    e.eval_spline_device(cd.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    Jd, gd = Jd.cpu().numpy(), _c3(gd.cpu().numpy(), ns, nu)
    # the same controls built in numpy
    u = np.einsum("tn,bnj->bjt", Bs, _c3(c, ns, nu))  # (B, nu, Nt)
    Ju, gu = blkseg_util.eval_dev(e, u)
    e.close()
    for a in (J, g, Jd, gd, Ju, gu):
        assert np.isfinite(a).all()
    ref = np.einsum("tn,bjt->bnj", Bs, gu)  # Bs' dJdu' per seed, (B, ns, nu)
    nrm = np.sqrt((ref ** 2).sum((1, 2)))
    assert (nrm > 0).all()
    dJ = np.abs(J - Ju).max()
    dJd = np.abs(Jd - Ju).max()
    rel = (np.sqrt(((g - ref) ** 2).sum((1, 2))) / nrm)
    reld = (np.sqrt(((gd - ref) ** 2).sum((1, 2))) / nrm)
    print(f"{name}: max |J - J(u)| = {dJ:.3e} (device form {dJd:.3e}), max rel dJdc = {rel.max():.3e} at seed "
          f"{int(rel.argmax())} (device form {reld.max():.3e} at seed {int(reld.argmax())})")
    assert dJ <= 1e-12 and dJd <= 1e-12
    assert rel.max() <= 1e-10 and reld.max() <= 1e-10
    for b in sorted({0, B // 2, B - 1}):
        Jr, gr = O.spline_eval(prob.A0, prob.A, Bs, c[b], prob.x0, prob.x_target, prob.n, order=3)
        ro = np.linalg.norm(g[b].ravel(order="F") - gr) / np.linalg.norm(gr)
        print(f"  seed {b} against the oracle: |dJ| = {abs(J[b] - Jr):.3e}, rel dJdc = {ro:.3e}")
        assert abs(J[b] - Jr) <= 1e-12 and abs(Jd[b] - Jr) <= 1e-12
        assert ro <= 1e-10
        assert np.linalg.norm(gd[b].ravel(order="F") - gr) / np.linalg.norm(gr) <= 1e-10


# ---- k_spline_constraints ------------------------------------------------------------------------------------------
def _cons_longdouble(c, ns, nu):
    """g = [norm(c), norm(diff(c, dims=1))] and the 2 x nc Jacobian of one seed in numpy.longdouble; a zero norm has a
    zero row."""
    L = np.longdouble
    C = np.asarray(c, dtype=L).reshape(nu, ns)  # row j: control j, index s
    D = np.diff(C, axis=1)
    g0, g1 = np.sqrt((C * C).sum()), np.sqrt((D * D).sum())
    Dp = np.zeros((nu, ns + 1), dtype=L)
    Dp[:, 1:ns] = D
    j0 = (C / g0 if g0 > 0 else np.zeros_like(C)).ravel()
    j1 = ((Dp[:, :ns] - Dp[:, 1:]) / g1 if g1 > 0 else np.zeros_like(C)).ravel()
    return np.array([g0, g1]), np.stack([j0, j1])


def _constraints_on_device(c, ns, nu):
    """k_spline_constraints through qoc_spline_constraints_dev on an engine with nu controls and ns splines."""
    from qoc_amd import GrapeEngine
    B, Nt = c.shape[0], 4
    prob = blkseg_util.block_problem(2, 2, nu, 1, Nt=Nt, seed=9)[0]
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    e.set_spline_basis(np.ones((Nt, ns)))
    cd = torch.from_numpy(np.ascontiguousarray(c)).to(DEV)
    gv = torch.full((B, 2), np.nan, dtype=torch.float64, device=DEV)
    gj = torch.full((B, 2, ns * nu), np.nan, dtype=torch.float64, device=DEV)
    g_only = torch.full((B, 2), np.nan, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    e.spline_constraints_device(cd.data_ptr(), gv.data_ptr(), gj.data_ptr())
    e.spline_constraints_device(cd.data_ptr(), g_only.data_ptr())  # the values alone (no Jacobian buffer)
    e.synchronize()
    e.close()
    assert torch.equal(gv, g_only)
    return gv.cpu().numpy(), gj.cpu().numpy()


def _check_constraints(tag, c, ns, nu):
    nc = ns * nu
    g, gj = _constraints_on_device(c, ns, nu)
    assert np.isfinite(g).all() and np.isfinite(gj).all()
    worst_g = worst_j = 0.0
    for b in range(c.shape[0]):
        gr, jr = _cons_longdouble(c[b], ns, nu)
        cmax = np.abs(c[b]).max()
        for i in range(2):
            if gr[i] == 0:
                assert g[b, i] == 0.0 and (gj[b, i] == 0.0).all(), (tag, b, i)
                continue
            eg = float(abs(g[b, i] - gr[i]) / gr[i])
            bound = (nc + 4) * EPS * np.abs(jr[i]) + EPS * cmax / gr[i]
            ej = float((np.abs(gj[b, i] - jr[i]) / bound).max())
            worst_g, worst_j = max(worst_g, eg / (nc * EPS)), max(worst_j, ej)
            assert eg <= nc * EPS, (tag, b, i, eg)
            assert ej <= 1.0, (tag, b, i, ej)
    print(f"{tag}: norm error / (nc eps) = {worst_g:.3f}, Jacobian error / bound = {worst_j:.3f}")
    return g, gj


def test_constraints_second_pass(built_lib):
    """(ns, nu) = (70, 4): nc = 280 > 256 threads, the second pass of both loops of k_spline_constraints.
    Measured on the MI355X: norm error 0.001 of nc eps, Jacobian error 0.039 of its bound."""
    c = 0.3 * np.random.default_rng(11).standard_normal((3, 280))
    g, _ = _check_constraints("ns70_nu4", c, 70, 4)
    assert (g > 0).all()


def test_constraints_one_spline(built_lib):
    """(ns, nu) = (1, 3): no differences, g1 = 0 and its Jacobian row exactly 0 (the g1 > 0.0 ? ... : 0.0 branch), not
    NaN; the norm row as usual.  Measured on the MI355X: norm error 0.18 of nc eps, Jacobian error 0.11 of its bound."""
    c = 0.3 * np.random.default_rng(12).standard_normal((2, 3))
    g, gj = _check_constraints("ns1_nu3", c, 1, 3)
    assert (g[:, 1] == 0.0).all() and (gj[:, 1] == 0.0).all() and (g[:, 0] > 0).all()


def test_constraints_zero_norms(built_lib):
    """(ns, nu) = (10, 2): a seed with c = 0 (both norms 0, both rows exactly 0), a seed constant along s
    (g1 = 0 with g0 > 0: row 1 exactly 0, row 0 c / g0), beside an ordinary seed.  Measured on the MI355X: norm error
    0.008 of nc eps, Jacobian error 0.033 of its bound."""
    c = 0.3 * np.random.default_rng(13).standard_normal((3, 20))
    c[1] = 0.0
    c[2] = np.repeat([0.37, -0.11], 10)  # index s + ns j: each control constant along s
    g, gj = _check_constraints("ns10_nu2", c, 10, 2)
    assert (g[0] > 0).all() and (gj[0] != 0).any()
    assert (g[1] == 0.0).all() and (gj[1] == 0.0).all()
    assert g[2, 0] > 0 and g[2, 1] == 0.0 and (gj[2, 1] == 0.0).all() and (gj[2, 0] != 0).all()
