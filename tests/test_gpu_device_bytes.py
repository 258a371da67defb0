"""info()["device_bytes"] (qoc_get_info's info[3]) after every op of a call sequence, against the recorded list in
tests/golden/device_bytes.json.  The values are integers and the comparison is exact: a change in how the context
allocates, counts or frees its device buffers moves a row.

The sequences: every one of engine_model.PINNED and the first 12 ops of a generated sequence on the dense cavity (the
Runner of tests/test_gpu_call_sequences.py, which also holds every value to the oracle), and short hand-written ones at
B = 2 and Nt <= 24 for the allocation sites those do not reach (HAND below).  No size in them depends on the free device
memory: every budget is cut to min(units, ...) first.

A pull request that changes what info[3] counts on purpose regenerates the file on an MI355X, from the repository's
root after a build:

    python tests/test_gpu_device_bytes.py

and shows the rows that moved in its diff.
"""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # run as a script: the import paths tests/conftest.py sets under pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "quantumoptimalcontrol.jl_amd"), os.path.join(_root, "oracle"),
                    os.path.join(_root, "tests")]

import engine_model as M  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_bytes.json")
B, NT = 2, 24


class BytesRunner(M.Runner):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.bytes = []

    def _route(self, op):
        self.bytes.append(self.e.info()["device_bytes"])
        return super()._route(op)


RUNNER = {name: so for name, so in M.PINNED.items()}
RUNNER["cavity_dense_first_12"] = ("cavity_dense", M.gen_ops("cavity_dense", M.SEEDS["cavity_dense"][0])[:12])


# ----------------------------------------------------------------------------------------------------------------------
# The hand-written sequences: each returns the byte count after the constructor and after every later op
# ----------------------------------------------------------------------------------------------------------------------
class _Rec:
    """An engine whose byte count is noted after every call made through it."""

    def __init__(self, mp, A0, A, x0, Nt, precision="fp64", **env):
        from qoc_amd import GrapeEngine
        for k in [k for k in os.environ if k.startswith("QOC_")]:
            mp.delenv(k)
        for k, v in env.items():
            mp.setenv(k, v)
        self.e = GrapeEngine(A0, A, x0, Nt, B=B, precision=precision)
        self.rows = [self.e.info()["device_bytes"]]

    def __call__(self, name, *a, **kw):
        out = getattr(self.e, name)(*a, **kw)
        self.rows.append(self.e.info()["device_bytes"])
        return out

    def eval(self, u, order):
        """eval_device on torch buffers, synchronised."""
        import torch
        ud = torch.from_numpy(np.array(np.transpose(u, (0, 2, 1)), order="C")).cuda()
        Jd = torch.zeros(B, dtype=torch.float64, device="cuda")
        gd = torch.zeros((B,) + ud.shape[1:], dtype=torch.float64, device="cuda")
        self("eval_device", ud.data_ptr(), order, Jd.data_ptr(), gd.data_ptr())
        self.e.synchronize()

    def done(self):
        self.e.close()
        return self.rows


def _cavity(nc=4, dense=False):
    from qoc_amd import systems
    return (systems.cavity_dense_problem if dense else systems.cavity_problem)(N_cavity=nc, Nt=NT)


def _u(seed):
    from qoc_amd import systems
    return systems.cavity_controls(B, NT, seed=seed)


def _x0_per_seed(prob):
    f = np.exp(1j * np.array([0.3, -1.1]))[:, None, None]
    return prob.x0[None] * f


def _fp32_stage(mp, **env):
    """A per-seed set_x0 after set_generators: the fp32 staging buffer grows to B N m elements."""
    p = _cavity()
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt, precision="fp32", **env)
    r("set_generators", p.A0, [0.5 * a for a in p.A])
    r("set_x0", _x0_per_seed(p), per_seed=True)
    r("set_cost_trace", p.x_target, p.n)
    r("propagate", _u(1))
    r("grape_sensitivity", _u(1), 3)
    r("state", NT, seed=1)
    return r.done()


def _fp32_large_n(mp):
    """The same on the large-N pipeline: the order-3 gradient's partial traces."""
    return _fp32_stage(mp, QOC_FORCE_LARGE_N="1")


def _exact_dense(mp):
    """The exact gradient on dense generators: the series' term counts and its workspace, grown on first use."""
    p = _cavity(dense=True)
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt)
    r("set_cost_trace", p.x_target, p.n)
    r("propagate", _u(2))
    r("grape_sensitivity", _u(2), "exact")
    r("grape_sensitivity", _u(2), "exact")
    r.eval(_u(3), "exact")
    return r.done()


def _spline_twice(mp):
    from qoc_amd import systems
    p = _cavity()
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt)
    r("set_cost_trace", p.x_target, p.n)
    rng = np.random.default_rng(4)
    for ns in (5, 9):
        r("set_spline_basis", systems.spline_matrix(float(NT), NT, ns))
        r("eval_spline", rng.uniform(-0.05, 0.05, size=(B, ns, 2)), 3)
    return r.done()


def _envelope(mp):
    import envgrad_util as E
    A0, A = E.transmon()
    x0 = np.eye(4, dtype=complex)[:, :2]
    r = _Rec(mp, A0, A, x0, 1)
    r("set_cost_trace", np.eye(4, dtype=complex)[:, [1, 0]], 2)
    P = np.array([[20.0, 5.0, 0.16, 0.4], [20.0, 4.0, 0.13, -0.2]])
    r("eval_envelope", "drag", P, 20.0, 0.05)
    r("propagate_envelope", "drag", P, 20.0, 0.05)
    return r.done()


def _costate_source(mp):
    p = _cavity()
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt)
    r("set_cost_trace", p.x_target, p.n)
    rng = np.random.default_rng(5)
    shape = (B, NT + 1, p.N, p.m)
    r("set_costate_source", 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)))
    r("propagate", _u(6))
    r("grape_sensitivity", _u(6), 3)
    r("set_costate_source", None)
    r.eval(_u(6), 3)
    return r.done()


def _compression(mp):
    """tests/test_gpu_compress.py's layout on the tunable bus: 4 columns packed into 2, and back."""
    from qoc_amd import systems
    p = systems.tunable_bus_cz_problem(Nt=NT, tgate=350.0 * NT / 2000)
    u = systems.tunable_bus_controls(B, NT, seed=3)
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt)
    r("set_cost_trace", p.x_target, p.n)
    r("propagate", u)
    r("set_compression", systems.TUNABLE_BUS_PARITY)
    r("propagate", u)
    r("grape_sensitivity", u, 3)
    r("set_compression", None)
    r("propagate", u)
    return r.done()


def _ensemble(mp):
    from qoc_amd import systems
    p = _cavity()
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt, QOC_ENS_SKIP="1")
    r("set_cost_trace", p.x_target, p.n)
    b = systems.annihilation_op(2)
    D = -1j * np.kron(b.T @ b, np.eye(4))
    A0s, As = systems.ensemble_members(p, dA0=[d * D for d in (0.0, 2e-3, -2e-3)], amp_scales=(1.0, 0.97, 1.04))
    r("set_generator_ensemble", A0s, As, (0.5, 0.3, 0.2))
    r("set_ensemble_objective", "cvar", 0.4)
    r.eval(_u(8), 3)
    r("set_ensemble_objective", "max")
    r.eval(_u(8), 3)
    r("clear_generator_ensemble")
    r.eval(_u(8), 3)
    return r.done()


def _time_scale(mp):
    p = _cavity()
    r = _Rec(mp, p.A0, p.A, p.x0, p.Nt)
    r("set_cost_trace", p.x_target, p.n)
    r("set_time_scale", np.array([0.8, 1.3]))
    r.eval(_u(9), 3)
    r("set_time_scale", None)
    r.eval(_u(9), 3)
    return r.done()


HAND = {"fp32_stage_grows": _fp32_stage, "fp32_large_n_order_3": _fp32_large_n, "exact_on_dense_cavity": _exact_dense,
        "spline_basis_twice": _spline_twice, "eval_envelope": _envelope, "costate_source": _costate_source,
        "set_compression": _compression, "ensemble_cvar_max_clear": _ensemble, "time_scale_set_eval_clear": _time_scale}
CASES = list(RUNNER) + list(HAND)


def record(name, mp):
    if name in HAND:
        return HAND[name](mp)
    sysname, ops = RUNNER[name]
    r = BytesRunner(sysname, ops, mp, tag=name).run()
    assert len(r.bytes) == len(ops)
    return r.bytes


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_bytes(built_lib, monkeypatch, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = record(name, monkeypatch)
    print(name, got)
    assert got == want, (name, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w], len(got), len(want))


def test_golden_file_names_every_case():
    with open(GOLDEN) as f:
        assert sorted(json.load(f)) == sorted(CASES)


if __name__ == "__main__":
    import torch
    torch.empty(1, device="cuda")  # torch's HIP runtime first, as tests/conftest.py built_lib
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rows = {name: record(name, M._Environ) for name in CASES}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{name}": {json.dumps(v)}' for name, v in rows.items()) + "\n}\n")
    print("wrote", out)
