"""Call sequences on one live context against the stateless model of tests/engine_model.py: what the engine keeps
between calls (lazily rebuilt states and co-states, a split forward's leftovers, the interpolation coefficients and their
control range, the live / dead block layout, launch shapes and penalty masks, the best-(J, seed) epilogue, captured
products, the host copies of the stale check) is right only while every setter and entry point drops exactly what it
must.  A sequence of ops (engine_model.gen_ops from numpy's default_rng, and the hand-written engine_model.PINNED) runs
on a GrapeEngine and on the model; after every op the two are compared:

    J, dJdu        per seed |dJ| <= 1e-12, ||d dJdu|| <= 1e-10 ||dJdu|| (tests/blkseg_util.assert_seed's bar); under
                   the z-calibrated cost the gradient and the co-states against the oracle's family in the calibration
                   phase (tests/test_gpu_parity.py::test_zcalibrated_cost: residual <= 1e-10, the phase within
                   qoc_oracle.zcal_dtheta_bound)
    x_k, lambda_k  max |d| <= 1e-12 max_k |value| (tests/test_gpu_blkseg.py::
                   test_lazy_states_survive_setters_and_later_calls)
    dead rows      exactly 0.0 where a pinned sequence says so
    allgather_best equal to (J.min(), offset + argmin) of the J the engine returned itself
    errors         the exception class and code; the reference's message for a stale u
    routes         the pinned sequences only: after every op info()'s backward, split_forward, fwd_captured,
                   interp_degree and interp_chain and the launches per phase since the op before, equal to the rows of
                   tests/golden/call_sequence_routes.json (engine_model.pinned_routes says how it is regenerated)

On a mismatch the failure names the system, the seed and the op, and prints the sequence so far as the literal that
PINNED takes.  The systems, all at B = 3 in fp64 (default environment plus QOC_BLOCKS=1): cavity20 (10 blocks of 2 rows,
Nt = 43), zz (3 blocks of 3 rows, Nt = 24), tunable_bus (parity blocks of 14 + 13 rows, one dead, Nt = 21),
tunable_bus_cz (both live, m = 4) and cavity_dense (no blocks: the Taylor-action chains), every one at the bar above.
"""
import numpy as np
import pytest

import engine_model as M

GENERATED = [(name, seed) for name in M.SYSTEMS for seed in M.SEEDS[name]]


@pytest.mark.gpu
@pytest.mark.parametrize("system,seed", GENERATED)
def test_generated_sequence(built_lib, monkeypatch, system, seed):
    ops = M.gen_ops(system, seed)
    r = M.Runner(system, ops, monkeypatch, tag=f"seed {seed}").run()
    assert r.ncmp == len(ops) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.PINNED))
def test_pinned_sequence(built_lib, monkeypatch, name):
    system, ops = M.PINNED[name]
    r = M.Runner(system, ops, monkeypatch, tag=name).run()
    assert r.ncmp == len(ops)
    want = M.pinned_routes()[name]  # no op on another path, none with a launch more, than when the file was written
    assert len(r.trace) == len(want)
    for i, (got, row) in enumerate(zip(r.trace, want)):
        assert got == row, (name, i, ops[i], "route", got, "recorded", row)


def test_sequences_cover_the_transitions():
    """Over each system's seed list: every setter class directly followed by each of eval, propagate, sensitivity,
    state and costate; eval, propagate_device and propagate each directly followed by a sensitivity with a stale u;
    eval, propagate, costate in a row; on the tunable bus the control ranges narrow, wide, narrow and (any), zero; and
    in every sequence of a system with a fast path an eval the model expects on it."""
    for name in M.SYSTEMS:
        assert 4 <= len(M.SEEDS[name]) <= 6
        pairs, fine = M.required_pairs(name)
        assert len(pairs) == 5 * len(M.setters_of(M.system(name))) and len(fine) == 3
        assert M.missing_transitions(name, [M.gen_ops(name, seed) for seed in M.SEEDS[name]]) == [], name
    assert "set_basis" in M.setters_of(M.system("zz")) and "set_basis" not in M.setters_of(M.system("cavity20"))


def test_generator_is_reproducible_and_weighted():
    """The same sequence from the same seed, 40 ops, about a third of them setters, every order and every op kind
    in use."""
    kinds, orders = set(), set()
    for name, seed in GENERATED:
        ops = M.gen_ops(name, seed)
        assert ops == M.gen_ops(name, seed) and len(ops) == 40
        nset = sum(op[0].startswith("set_") or op[0] == "comm" for op in ops)
        assert 8 <= nset <= 20, (name, seed, nset)
        kinds |= {op[0] for op in ops}
        orders |= {op[2] for op in ops if op[0].startswith(("eval", "sens"))}
    assert orders == set(M.ORDERS)
    assert kinds == {"set_gen", "set_x0", "set_cost", "set_pen", "set_src", "set_basis", "comm", "eval", "eval_spl", "prop",
                     "prop_dev", "prop_spl", "sens", "sens_dev", "sens_spl", "state", "costate", "best"}


def test_model_predicts_every_op():
    """The model run over every generated and pinned sequence: a prediction for each op (never "unknown"), as many
    as there are ops, and an error leaves the model as it was."""
    seqs = [(name, M.gen_ops(name, seed)) for name, seed in GENERATED] + list(M.PINNED.values())
    nerr = 0
    for name, ops in seqs:
        m = M.Model(name)
        preds = []
        for op in ops:
            before = (m.st, m.fwd, m.bwd, m.jfwd)
            p = m.apply(op)
            assert p.kind in ("ok", "err", "J", "g", "Jg", "x", "lam", "best"), (name, op, p.kind)
            if p.kind == "err":
                nerr += 1
                assert (m.st, m.fwd, m.bwd, m.jfwd) == before
                assert p.code in (M.ERR_ARG, M.ERR_STALE, M.ERR_STATE) and p.stale == (p.code == M.ERR_STALE)
            preds.append(p)
        assert len(preds) == len(ops)
    assert nerr > 0


def test_model_values_are_the_oracles():
    """The model's values are the oracle's from scratch on the snapshot: one short zz sequence against direct calls of
    qoc_oracle (the penalty set after the propagate enters the sensitivity, not the propagate's J)."""
    import qoc_oracle as O
    s = M.system("zz")
    m = M.Model("zz")
    pJ = m.apply(("prop", "u1"))
    m.apply(("set_pen", "pen0"))
    pg = m.apply(("sens", "u1", 3))
    px = m.apply(("state", 5, 2))
    pl = m.apply(("costate", 5, 2))
    m.apply(("set_cost", "trace_neg"))
    assert m.apply(("state", 5, 2)).kind == "err" and m.apply(("costate", 5, 2)).bwd == pl.bwd
    A0, A = s.gens["g0"]
    u = s.ctrls["u1"]
    kind, xt, n = s.costs["trace"]
    for b in range(M.B):
        J0, _, _ = O.grape_eval(A0, A, u[b], s.x0s["x0"][0], xt, n, order=3)
        _, g1, c1 = O.grape_eval(A0, A, u[b], s.x0s["x0"][0], xt, n, order=3, penalty=s.pens["pen0"])
        assert pJ.J()[b] == J0
        assert np.array_equal(pg.lam_g()[1][b], g1)
        if b == 2:
            assert np.array_equal(px.states()[2][5], c1.x[5]) and np.array_equal(pl.lam_g()[0][2][5], c1.lam[5])
