"""The fixed costs around the segmented block eval's two loops (csrc/qoc_blkseg.hpp, csrc/qoc_run_blkseg.hip): the
packed table of generator blocks that the host builds with the block layout and the prologue copies (it has to follow
qoc_set_generators), X_target staged in LDS for the cost section, the launch shape and the kernels' dynamic-LDS limit
kept in the context between evals, and the fence-free phase events.  Conventions and bars of
tests/test_gpu_blkseg.py: |ΔJ| <= 1e-12, ||ΔdJdu|| / ||dJdu|| <= 1e-10 per seed against the oracle.
"""
import dataclasses
import time

import numpy as np
import pytest

import qoc_oracle as O
from blkseg_util import assert_seed as _assert_seed, block_problem as _block_problem
from blkseg_util import engine as _engine, eval_dev as _eval_dev

pytestmark = pytest.mark.gpu


def _assert_oracle(prob, u, J, g, tag):
    for b in range(u.shape[0]):
        J0, g0, _ = O.grape_eval(prob.A0, prob.A, u[b], prob.x0, prob.x_target, prob.n, order=3)
        _assert_seed(J[b], g[b], J0, g0, (tag, b))


def _cavity20():
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=50)  # N = 20, 10 blocks of 2, m = 2
    return p, systems.cavity_controls(3, p.Nt, seed=282)


def _setter_cases():
    out = {"cavity20": _cavity20()}
    out["blocks2"] = _block_problem(2, 7, 1, 3, Nt=45, seed=711)[:2]
    out["blocks3"] = _block_problem(3, 5, 2, 2, Nt=45, seed=712)[:2]
    return out


@pytest.mark.parametrize("name", ["cavity20", "blocks2", "blocks3"])
def test_generator_blocks_follow_the_setters(built_lib, monkeypatch, name):
    """The packed table of generator blocks follows qoc_set_generators (the sizes stay, so the kept launch shape is
    reused while the table is rebuilt): an eval, the control generators scaled through the setter, an eval again; each
    against the oracle for its own generators.  Blocks of 2 rows, blocks of 2 with a padded row (zeros in the table),
    blocks of 3."""
    prob, u = _setter_cases()[name]
    e = _engine(prob, u.shape[0], monkeypatch)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    scale = (1.7, 0.6)
    p2 = dataclasses.replace(prob, A=[a * scale[j] for j, a in enumerate(prob.A)])
    e.set_generators(p2.A0, p2.A)
    J2, g2 = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    _assert_oracle(prob, u, J, g, (name, "first"))
    _assert_oracle(p2, u, J2, g2, (name, "scaled"))


def test_one_block_differing_by_1e_9(built_lib, monkeypatch):
    """One block's control entry off by a relative 1e-9 (the generator kept exactly skew-Hermitian): the eval matches
    the oracle of these generators, so each block's own table entries are used."""
    prob, u = _cavity20()
    A1 = prob.A[0].copy()
    i, k = [(i, k) for i, k in zip(*np.nonzero(A1)) if i < k][-1]  # the last block's entry
    A1[i, k] *= 1.0 + 1e-9
    A1[k, i] = -np.conj(A1[i, k])
    assert A1[i, k] != prob.A[0][i, k] and np.array_equal(A1, -A1.conj().T)
    p2 = dataclasses.replace(prob, A=[A1] + list(prob.A[1:]))
    e = _engine(p2, u.shape[0], monkeypatch)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    _assert_oracle(p2, u, J, g, "one block differs")


def test_controls_buffer_not_16_byte_aligned(built_lib, monkeypatch):
    """Two controls are read with one 16-byte load per slice when the caller's buffer allows it: a buffer that starts 8
    bytes off takes the 8-byte loads and gives the same bits."""
    import torch
    prob, u = _cavity20()
    B, nu, Nt = u.shape
    e = _engine(prob, B, monkeypatch)
    J, g = _eval_dev(e, u)
    flat = torch.zeros(B * Nt * nu + 1, dtype=torch.float64, device="cuda")
    flat[1:] = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1))).reshape(-1)).cuda()
    assert (flat.data_ptr() + 8) % 16 == 8
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.empty(B, Nt, nu, dtype=torch.float64, device="cuda")
    e.eval_device(flat.data_ptr() + 8, 3, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    e.close()
    assert np.array_equal(Jd.cpu().numpy(), J)
    assert np.array_equal(np.transpose(gd.cpu().numpy(), (0, 2, 1)), g)
    _assert_oracle(prob, u, J, g, "aligned")


@pytest.mark.parametrize("amp", [8.0, 14.0])
def test_series_degree_classes_7_and_9(built_lib, monkeypatch, amp):
    """The K = 7 and K = 9 series classes (amplitudes of test_segmented_series_degree_classes) through the new
    prologue, against the oracle."""
    from qoc_amd import systems
    p = systems.cavity_problem(N_cavity=10, Nt=40)
    u = systems.cavity_controls(3, p.Nt, seed=91) * amp
    e = _engine(p, 3, monkeypatch)
    J, g = _eval_dev(e, u)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    _assert_oracle(p, u, J, g, ("amp", amp))


@pytest.mark.parametrize("registered", [False, True])
@pytest.mark.parametrize("B", [1, 65, 130])
def test_best_pair_over_consecutive_evals(built_lib, monkeypatch, B, registered):
    """The last workgroup's reduction of J on one engine over consecutive evals with different u (the counter is reset
    by each launch) and a propagate between them: one workgroup, then one and two wraps of the 64-lane read loop; two
    seeds with the same u (the lower index wins); with and without a registered output buffer."""
    import torch
    from qoc_amd import systems
    prob = systems.cavity_problem(N_cavity=10, Nt=24)
    u = systems.cavity_controls(B, prob.Nt, seed=291) * 6.0  # spread the fidelities
    e = _engine(prob, B, monkeypatch)
    best_d = torch.full((2,), np.nan, dtype=torch.float64, device="cuda")
    if registered:
        e.set_best_output(best_d.data_ptr())

    def check(uu, tag):
        J, _ = _eval_dev(e, uu)
        assert e.info()["backward"] == "segmented", e.info()
        want = (J.min(), int(np.argmin(J)))
        if registered:
            e.allgather_best_device(best_d.data_ptr())
            e.synchronize()
            got = best_d.cpu().numpy()
            assert (got[0], int(got[1])) == want, (tag, got, want)
        assert e.allgather_best() == want, tag
        return J

    J = check(u, "first")
    check(u[::-1].copy(), "reversed")
    Jp = e.propagate(u * 0.25)  # the forward half alone publishes too
    assert e.allgather_best() == (Jp.min(), int(np.argmin(Jp)))
    u3 = u * 0.5
    if B > 1:  # a tie at the minimum: the seed after the best one (cyclically) gets its u
        i = int(np.argmin(check(u3, "probe")))
        k = (i + 1) % B
        u3 = u3.copy()
        u3[k] = u3[i]
        J3 = check(u3, "tie")
        assert J3[i] == J3[k] == J3.min() and int(np.argmin(J3)) == min(i, k)
    else:
        check(u3, "third")
    e.close()


def test_phase_times_of_the_one_launch_eval(built_lib, monkeypatch):
    """With profiling on, K evals of the fused form count K launches in k_chain_bwd alone, with a total that is positive
    and within the host's wall time around the synchronised loop; the split form counts k_chain_fwd and k_chain_bwd."""
    import torch
    prob, u = _cavity20()
    B, nu, Nt = u.shape
    K = 5
    e = _engine(prob, B, monkeypatch)
    ud = torch.from_numpy(np.ascontiguousarray(np.transpose(u, (0, 2, 1)))).cuda()
    Jd = torch.empty(B, dtype=torch.float64, device="cuda")
    gd = torch.empty(B, Nt, nu, dtype=torch.float64, device="cuda")
    e.eval_device(ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())  # (first-use allocations stay outside)
    e.synchronize()
    e.phase_times(reset=True)
    e.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(K):
        e.eval_device(ud.data_ptr(), 3, Jd.data_ptr(), gd.data_ptr())
    e.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    ph = e.phase_times(reset=True)
    print("fused", ph, "wall ms", wall_ms)
    assert ph["k_chain_bwd"][1] == K and 0.0 < ph["k_chain_bwd"][0] <= wall_ms, (ph, wall_ms)
    assert all(ph[k][1] == 0 and ph[k][0] == 0.0 for k in ("k_expm", "k_chain_fwd", "k_grad")), ph
    for _ in range(K):
        e.propagate_device(ud.data_ptr(), Jd.data_ptr())
        e.grape_sensitivity_device(ud.data_ptr(), 3, gd.data_ptr())
    e.synchronize()
    ph = e.phase_times(reset=True)
    e.set_profiling(False)
    assert e.info()["split_forward"] == "segmented", e.info()
    e.close()
    print("split", ph)
    assert ph["k_chain_fwd"][1] == K and ph["k_chain_bwd"][1] == K, ph
    assert ph["k_chain_fwd"][0] > 0.0 and ph["k_chain_bwd"][0] > 0.0, ph


def test_launch_shape_kept_between_evals_follows_its_inputs(built_lib, monkeypatch):
    """The launch shape is derived once per context: two evals on one engine agree bit for bit, an engine built under
    another QOC_BLKSEG_S agrees with them to the parity bars, and a context whose generators are replaced by ones with
    another block count (20 rows: 10 blocks of 2, then 6 blocks of 3 and one of 2) evaluates those correctly."""
    prob, u = _cavity20()
    B = u.shape[0]
    e = _engine(prob, B, monkeypatch)
    J, g = _eval_dev(e, u)
    Jb, gb = _eval_dev(e, u)
    assert np.array_equal(J, Jb) and np.array_equal(g, gb)
    e7 = _engine(prob, B, monkeypatch, S=7)
    J7, g7 = _eval_dev(e7, u)
    e7.close()
    for b in range(B):
        _assert_seed(J7[b], g7[b], J[b], g[b], ("S=7", b))
    _assert_oracle(prob, u, J, g, "S default")
    pb, _, _ = _block_problem(3, 7, 2, 2, Nt=prob.Nt, seed=714)
    assert pb.N == prob.N
    p2 = dataclasses.replace(prob, A0=pb.A0, A=pb.A)
    e.set_generators(p2.A0, p2.A)
    ub = np.random.default_rng(5).uniform(-1, 1, size=u.shape)
    J2, g2 = _eval_dev(e, ub)
    assert e.info()["backward"] == "segmented", e.info()
    e.close()
    _assert_oracle(p2, ub, J2, g2, "blocks of 3")
