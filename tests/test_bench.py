"""bench.py's options beside the metric: --dump-outputs writes what the last timed step computed, --full gates the legs
that the headline figure does not need (CPU baseline, parity against it, side legs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_dtype_and_samples_large_arrays(tmp_path):
    """float32 stays float32, everything else becomes float64; an array above its share of the 64 MB limit is cut to
    the same seeded sample of its entries in every call."""
    import bench
    big = np.arange(5_000_000, dtype=np.float64).reshape(1000, 5000)  # 40 MB, above the 21 MB share of three arrays
    arrays = {"small32": np.linspace(0, 1, 7, dtype=np.float32), "ints": np.arange(4), "big": big}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays, rank=2)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["big.npy", "ints.npy", "small32.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == ["big.rank2.npy", "ints.rank2.npy", "small32.rank2.npy"]
    assert a["small32.npy"].dtype == np.float32 and np.array_equal(a["small32.npy"], arrays["small32"])
    assert a["ints.npy"].dtype == np.float64 and np.array_equal(a["ints.npy"], np.arange(4.0))
    assert a["big.npy"].dtype == np.float64 and a["big.npy"].ndim == 1
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES
    assert a["big.npy"].size == bench.DUMP_MAX_BYTES // 3 // 8
    assert np.all(np.diff(a["big.npy"]) > 0)  # entries of arange: distinct indices, in order
    assert np.array_equal(a["big.npy"], np.load(tmp_path / "b" / "big.rank2.npy"))


def _bench(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                         text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_leaves_the_full_legs_out(built_lib, tmp_path):
    """A plain run of the B = 1 zz config: the result line has the contract's keys and none of the --full legs; J,
    dJdu and best in the dump directory are the fused eval's outputs on the config's seeded controls (against the C
    port at the fp64 bars of the parity tests)."""
    import cpuref
    from qoc_amd import systems
    rec = _bench("--config", "zz_plumbing", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "evals/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(1e3 / rec["ms_per_step"], rel=1e-9)  # B = 1
    assert rec["cpu_baseline"] is None and rec["parity_vs_cpu_port"] is None and "side_legs" not in rec
    mk_prob, mk_u, B = systems.CONFIGS["zz_plumbing"]
    prob, u = mk_prob(), mk_u(B, 0)
    J, g, best = (np.load(tmp_path / f) for f in ("J.npy", "dJdu.npy", "best.npy"))
    assert J.dtype == g.dtype == best.dtype == np.float64
    assert J.shape == (B,) and g.shape == (B, prob.Nt, prob.nu) and best.shape == (2,)
    cpuref.use_blas(False)
    Jc, gc = cpuref.grape_eval_batch(prob, u, order=3, mode=0)
    assert np.abs(J - Jc).max() <= 1e-12
    gt = np.transpose(g, (0, 2, 1))
    assert max(np.linalg.norm(gt[b] - gc[b]) / np.linalg.norm(gc[b]) for b in range(B)) <= 1e-10
    assert best[0] == J.min() and best[1] == float(np.argmin(J))


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline_and_the_side_legs(built_lib):
    """--full on the same config: the CPU baseline with its parity check, and the side leg that --side names."""
    rec = _bench("--config", "zz_plumbing", "--steps", "3", "--warmup", "1", "--full", "--cpu-seconds", "0.2",
                 "--side", "zz_plumbing:split")
    assert rec["cpu_baseline"]["value"] > 0 and rec["speedup_vs_cpu"] > 0
    assert rec["parity_vs_cpu_port"]["max_abs_dJ"] <= 1e-12 and rec["parity_vs_cpu_port"]["max_rel_dJdu"] <= 1e-10
    leg = rec["side_legs"]["zz_plumbing:split"]
    assert leg["value"] > 0 and leg["steps"] == 5
    assert leg["parity_vs_cpu_port"]["max_abs_dJ"] <= 1e-12 and leg["parity_vs_cpu_port"]["max_rel_dJdu"] <= 1e-10
