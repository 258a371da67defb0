"""The exact gradient on dense generators as a series on MFMA (csrc/qoc_grad_rr.hpp k_grad_rr_xn / _xq / _xp, routed by
qoc_run_grad.hip grad_rr_exact): dUkdp_order = "exact" on contexts without a block path (QOC_BLOCKS=0) that the fused
gradient kernels fit.

The bar is the project's fp64 bar against oracle/qoc_oracle.grape_eval(..., order="exact"), one block
exponential per slice and control: |ΔJ| <= 1e-12 and ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed.  exact_series_stats() tells
which route ran: the (seed, slice) units the series kernels processed, their term counts, the calls that fell back to
the block exponential.  The term-count rule and the generators' bounds are restated in tests/gradx_util.py.
"""
import functools

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import assert_seed as _assert_seed, engine as _block_engine, eval_dev as _eval_dev, split_dev as _split_dev
from gradx_util import GRADX_NMAX, exact_terms, gue_problem, rho_of, shifts

pytestmark = pytest.mark.gpu

EX = "exact"
SWITCHES = ("QOC_GRAD_EXACT_SERIES", "QOC_GRAD_EXACT_WS_MB", "QOC_BLKSEG_EXACT", "QOC_BLKP_EXACT", "QOC_BLKSEG")


def _engine(prob, B, monkeypatch, chain=None, env=None, cost="trace"):
    """A dense context: no block path whatever the generators' structure (QOC_BLOCKS=0 at qoc_set_generators)."""
    from qoc_amd import GrapeEngine
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("QOC_BLOCKS", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    e = GrapeEngine(prob.A0, prob.A, prob.x0, prob.Nt, B=B)
    if cost == "trace":
        e.set_cost_trace(prob.x_target, prob.n)
    elif cost == "zcal":
        e.set_cost_zcalibrated(prob.x_target)
    else:
        e.set_cost_external()
    if chain is not None:
        e.set_chain(chain)
        assert e.info()["chain"] == chain
    assert e.info()["chain_kernel"] not in ("blocks", "blocks_mfma", "blocks_prop", "blocks_prop16")
    return e


def _oracle_all(prob, u, penalty=None):
    return tuple(O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=EX, penalty=penalty)[:2]
                 for b in range(u.shape[0]))


def _assert_all(J, g, ref, tag):
    for b in range(len(ref)):
        _assert_seed(J[b], g[b], ref[b][0], ref[b][1], tag + (b,))


def _bound(e, prob):
    """The per-generator bound the engine's term counts use: spectral half-widths where the Chebyshev chains apply,
    1-norms of the shifted generators otherwise."""
    _, rad, nrm = shifts(prob)
    return rad if e.info()["chain_poly"] == "chebyshev" else nrm


def _n_max(bound, u):
    return max(exact_terms(r) for b in range(u.shape[0]) for r in rho_of(bound, u[b]))


# ---- 1. shapes ------------------------------------------------------------------------------------------------------
SHAPES = {4: 7, 9: 13, 20: 9}  # N_cavity -> Nt: N = 8, 18, 40 (NT = 1, 2, 3; last row tile of 2, 1, 2 valid quads)


@functools.lru_cache(maxsize=None)
def _shape_case(nc):
    from qoc_amd import systems
    prob = systems.cavity_dense_problem(nc, SHAPES[nc])
    u = systems.cavity_controls(3, prob.Nt, seed=40 + nc)
    return prob, u, _oracle_all(prob, u)


@pytest.mark.parametrize("chain", ["taylor", "propagators"])
@pytest.mark.parametrize("nc", sorted(SHAPES))
def test_shapes_both_chains_both_call_forms(built_lib, monkeypatch, nc, chain):
    """B = 3: 21, 39 and 27 units of m = 2 columns, eight units per tile, each ending in a ragged last tile."""
    prob, u, ref = _shape_case(nc)
    B, Nt = u.shape[0], prob.Nt
    assert (B * Nt) % 8 != 0
    e = _engine(prob, B, monkeypatch, chain=chain)
    for form in (_eval_dev, _split_dev):
        J, g = form(e, u, EX)
        st = e.exact_series_stats(reset=True)
        assert st["units"] == B * Nt and st["fallbacks"] == 0, (form.__name__, st)
        assert Nt * B <= st["terms"] <= st["n_max"] * B * Nt and 1 <= st["n_max"] <= GRADX_NMAX, st
        _assert_all(J, g, ref, (nc, chain, form.__name__))
    assert e.exact_series_stats() == {"units": 0, "terms": 0, "n_max": 0, "fallbacks": 0}
    # the cases tell the gradients apart: the oracle's order 3 is far outside the bar
    g3 = O.grape_eval(prob.A0, prob.A, u[0], prob.x0, prob.x_target, prob.n, order=3)[1]
    assert np.linalg.norm(g3 - ref[0][1]) / np.linalg.norm(ref[0][1]) > 1e-7
    # the ABI's argument check with a live context
    assert e._lib.qoc_exact_series_stats(e._h, None, 0) == -1
    e.close()


# ---- 2. tile edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("m", [1, 4, 16])
@pytest.mark.parametrize("N", [16, 32, 48, 33, 47])
def test_tile_edges_gue(built_lib, monkeypatch, N, m, nu):
    """GUE generators with 1-norm bounds ρ_k in [2, 2 + nu] (the spectral half-widths, which set the counts where the
    Chebyshev chains apply, lie near 1), Nt = 5, B = 2: full and ragged row tiles, 16, 4 and one unit per tile; N = 48 with
    m = 16 has no Taylor-action chains and takes its shifts and bounds without them."""
    prob, u = gue_problem(N, m, nu, 5, seed=1000 * N + 10 * m + nu)
    ref = _oracle_all(prob, u)
    e = _engine(prob, 2, monkeypatch)
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st["units"] == 10 and st["fallbacks"] == 0, st
    _assert_all(J, g, ref, (N, m, nu))


@functools.lru_cache(maxsize=None)
def _zz_case():
    from qoc_amd import systems
    prob = systems.zz_problem(20, tgate=2.0)
    return prob, systems.zz_controls(2, 20, 2.0, seed=77)


def test_zz_dense_state_penalty(built_lib, monkeypatch):
    """N = 9, m = 4 (four units per tile) with the guard-state penalty in J and in the co-states."""
    from qoc_amd import systems
    prob, u = _zz_case()
    qb = systems.QuantumBasis([3, 3])
    pen = ([int(r) for r in qb(["20", "21", "22"])], [0, 1, 2, 3], 0.37)
    ref = _oracle_all(prob, u, penalty=pen)
    e = _engine(prob, 2, monkeypatch)
    e.set_state_penalty(*pen)
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st["units"] == 2 * prob.Nt and st["fallbacks"] == 0, st
    _assert_all(J, g, ref, ("zz_pen",))


def test_zz_dense_zcalibrated(built_lib, monkeypatch):
    """The z-calibrated cost: J against the oracle's cost of its own x_N, the gradient against the oracle's exact
    gradient family g(Δθ) within the calibration phase's golden-section bound (tests/test_gpu_parity.py)."""
    prob, u = _zz_case()
    Jz, _ = O.setup_infidelity_zcalibrated(prob.x_target)
    e = _engine(prob, 2, monkeypatch, cost="zcal")
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st["units"] == 2 * prob.Nt and st["fallbacks"] == 0, st
    for b in range(2):
        xN = O.propagate(prob.A0, prob.A, u[b], prob.x0)[-1]
        assert abs(J[b] - Jz(xN)) <= 1e-12
        res, dth = O.zcal_gradient_match(g[b], prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=EX)
        assert res <= 1e-10 and abs(dth) <= O.zcal_dtheta_bound(prob.x_target, xN), (b, res, dth)


def test_external_lambda_final(built_lib, monkeypatch):
    """QOC_COST_EXTERNAL: the caller's λ_N (random, per seed) through the host call form."""
    prob, u = gue_problem(18, 2, 2, 6, seed=5)
    rng = np.random.default_rng(6)
    lamN = rng.standard_normal((2, prob.N, prob.m)) + 1j * rng.standard_normal((2, prob.N, prob.m))
    e = _engine(prob, 2, monkeypatch, cost="external")
    e.propagate(u)
    g = e.grape_sensitivity(u, EX, lambda_final=lamN)
    st = e.exact_series_stats()
    e.close()
    assert st["units"] == 12 and st["fallbacks"] == 0, st
    for b in range(2):
        cost = (lambda x: 0.0, lambda x, b=b: lamN[b])
        g0 = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, order=EX, cost=cost)[1]
        rel = np.linalg.norm(g[b] - g0) / np.linalg.norm(g0)
        assert rel <= 1e-10, (b, rel)


# ---- 3-5. mixed counts in one tile, range independence, the cap ------------------------------------------------------
RAMP_NT, RAMP_B = 40, 3


@functools.lru_cache(maxsize=None)
def _ramp_base():
    from qoc_amd import systems
    prob = systems.cavity_dense_problem(9, RAMP_NT)
    return prob, systems.cavity_controls(RAMP_B, RAMP_NT, seed=49)


def _ramp(bound):
    """The controls with a per-slice scale ramping linearly from 1 to the largest integer factor whose term counts stay
    within the cap (found here from the rule's restatement), and the restatement's largest count."""
    prob, u0 = _ramp_base()
    ramp = lambda f: u0 * np.linspace(1.0, f, RAMP_NT)[None, None, :]
    f = 1
    while _n_max(bound, ramp(f + 1)) <= GRADX_NMAX:
        f += 1
    assert f > 10
    return ramp(f), _n_max(bound, ramp(f))


@functools.lru_cache(maxsize=None)
def _ramp_oracle(key):
    prob, _ = _ramp_base()
    return _oracle_all(prob, np.frombuffer(key).reshape(RAMP_B, 2, RAMP_NT))


def test_mixed_term_counts_in_one_tile(built_lib, monkeypatch):
    """Neighbouring slices share a tile, so the counts within one tile differ: from about 12 at the first slice to the
    cap at the last."""
    prob, _ = _ramp_base()
    e = _engine(prob, RAMP_B, monkeypatch)
    u, n_want = _ramp(_bound(e, prob))
    assert n_want >= GRADX_NMAX - 4 and exact_terms(rho_of(_bound(e, prob), u[0])[0]) <= 16
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st["units"] == RAMP_B * RAMP_NT and st["fallbacks"] == 0, st
    assert abs(st["n_max"] - n_want) <= 1, (st, n_want)
    _assert_all(J, g, _ramp_oracle(u.tobytes()), ("ramp",))


def test_slice_ranges_leave_the_result_bitwise(built_lib, monkeypatch):
    """A workspace of 1 MiB holds 12 slices of the ramp case (48 x 3 x 18 x 2 x 16 bytes each): four slice ranges, whose
    tiles group other units than the one-range run's.  dJdu is bitwise the same."""
    prob, _ = _ramp_base()
    out = []
    for env in (None, {"QOC_GRAD_EXACT_WS_MB": "1"}):
        e = _engine(prob, RAMP_B, monkeypatch, env=env)
        u, n_want = _ramp(_bound(e, prob))
        out.append(_eval_dev(e, u, EX) + (e.exact_series_stats(),))
        e.close()
        per_slice = out[-1][2]["n_max"] * RAMP_B * prob.N * prob.m * 16
        assert RAMP_NT * per_slice > 3 * (1 << 20) > 0 and per_slice <= 1 << 20
    assert out[0][2] == out[1][2] and out[0][2]["units"] == RAMP_B * RAMP_NT
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    _assert_all(out[1][0], out[1][1], _ramp_oracle(u.tobytes()), ("ranges",))


def test_cap_falls_back_to_the_block_exponential(built_lib, monkeypatch):
    """The controls times the smallest integer that puts the largest count above the cap (ρ_max just above 8.6, far below
    the 16 the block exponential's own tests cover): the whole call runs the block exponential."""
    prob, u0 = _ramp_base()
    e = _engine(prob, RAMP_B, monkeypatch)
    bound = _bound(e, prob)
    s = 1
    while _n_max(bound, u0 * s) <= GRADX_NMAX:
        s += 1
    u = u0 * s
    assert max(rho_of(bound, u[b]).max() for b in range(RAMP_B)) < 16.0
    J, g = _eval_dev(e, u0 * (s - 1), EX)  # the last scale below the cap: the series
    st0 = e.exact_series_stats()
    assert st0["units"] == RAMP_B * RAMP_NT and st0["fallbacks"] == 0, st0
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st["fallbacks"] == 1 and st["units"] == st0["units"] and st["terms"] == st0["terms"], (st0, st)
    _assert_all(J, g, _oracle_all(prob, u), ("cap", s))


# ---- 6-7. the switch, block contexts ----------------------------------------------------------------------------------
def test_switch_keeps_the_block_exponential(built_lib, monkeypatch):
    prob, u, ref = _shape_case(9)
    e = _engine(prob, u.shape[0], monkeypatch, env={"QOC_GRAD_EXACT_SERIES": "0"})
    J, g = _eval_dev(e, u, EX)
    st = e.exact_series_stats()
    e.close()
    assert st == {"units": 0, "terms": 0, "n_max": 0, "fallbacks": 0}, st
    _assert_all(J, g, ref, ("switch",))


def test_block_contexts_keep_the_block_exponential(built_lib, monkeypatch):
    """zz with its blocks on and QOC_BLKSEG_EXACT=0: the exact eval reaches the dense gradient from a block context,
    which keeps the block exponential (the second implementation of tests/test_gpu_blkseg_exact.py)."""
    prob, u = _zz_case()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    e = _block_engine(prob, 2, monkeypatch, segex="0")
    J, g = _eval_dev(e, u, EX)
    assert e.info()["backward"] != "segmented"
    st = e.exact_series_stats()
    e.close()
    assert st == {"units": 0, "terms": 0, "n_max": 0, "fallbacks": 0}, st
    _assert_all(J, g, _oracle_all(prob, u), ("blocks",))
