"""bench.py as the driver runs it: `python bench.py --gpus N` starts its own ranks (no launcher), prints one JSON line
with the contract's keys, and can run the stated configurations (weak / strong scaling, an explicit global domain).  On a
1-GPU box the ranks share the device and the face exchange is host-staged (gloo)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "1", "--warmup", "1", "--nz", "16", "--no-cpu-baseline", "--kernel-reps", "2"]


def _run(args, env=None, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})), cwd=ROOT)
    return p


def _line(p):
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_one_gpu_line_has_the_contract_keys(gpu):
    out = _line(_run(["--nx", "64", "--ny", "32", "--full"] + SMALL))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "roofline_spmv", "roofline_iter", "roofline_pc"):
        assert k in out, k
    assert out["metric"].startswith("pprts 3_10") and out["n_gpus"] == 1 and out["scaling"] == "weak"
    assert out["config"]["reason"] in (2, 3)
    # the launch the solve spends most of its time in: the flow kernel (the intermediate passes of an application in ONE launch,
    # round 5) where it runs -- this domain: 64 x 32 columns, tiles of 16 -- with the single pass beside it
    assert "tsx_k_pcs_flow" in out["roofline"]["kernel"] and out["roofline"]["frac"] > 0
    assert out["config"]["flow_kernel"]["in_use"] and "tsx_k_pcs_rb" in out["roofline_pass"]["kernel"]
    assert out["roofline"]["passes_per_launch"] == out["config"]["flow_kernel"]["end_pass"] - out["config"]["flow_kernel"]["first_pass"]
    for k in ("first_solve", "step_ms_min_med_max", "no_hint"):
        assert k in out["config"], k
    # the metric names the solver that ran
    out8 = _line(_run(["--nx", "16", "--ny", "12", "--solver", "8_16", "--full"] + SMALL))
    assert out8["metric"].startswith("pprts 8_16") and "tsx_k_pcsh_rb" in out8["roofline"]["kernel"]
    for r in (out["roofline"], out["roofline_pass"], out["roofline_spmv"], out8["roofline"], out8["roofline_spmv"]):
        assert 0 < r["frac"] < 1, r   # bytes of the storage format in use: never above the peak


def test_plain_bench_times_its_steps_and_dumps_the_last_one(gpu, tmp_path):
    """Without --full: the headline keys and nothing measured beside them, --steps timed steps, and --dump-outputs writes what the
    last timed step computed (fp64, the whole solution at this size); two runs of the same arguments solve the same system."""
    args = ["--nx", "64", "--ny", "32", "--nz", "16", "--steps", "3", "--warmup", "1"]
    xs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = _line(_run(args + ["--dump-outputs", str(d)]))
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype",
                    "data", "config"):
            assert key in out, key
        assert "roofline" not in out and "cpu_baseline" not in out
        assert not {"tight_run", "no_hint", "no_sharing", "all_fp64", "heterogeneous"} & set(out["config"])
        assert out["steps"] == 3 and out["config"]["reason"] in (2, 3)
        assert out["value"] == pytest.approx(64 * 32 * 16 / (out["ms_per_step"] * 1e-3), rel=1e-9)
        assert sorted(os.listdir(d)) == ["residual_history.npy", "solve_info.npy", "x.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        info, x = np.load(d / "solve_info.npy"), np.load(d / "x.npy")
        assert info.dtype == x.dtype == np.float64 and x.shape == (32, 64, 17, 10)
        assert info[0] == out["config"]["iterations"] and info[1] == out["config"]["reason"]
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        xs.append(x)
    assert np.abs(xs[0] - xs[1]).max() <= 1e-6 * np.abs(xs[0]).max()


@pytest.mark.parametrize("extra,glob,local,scaling", [
    (["--nx", "32", "--ny", "24", "--scaling", "weak"], (32, 48), (32, 24), "weak"),
    (["--nx", "32", "--ny", "24", "--scaling", "strong"], (32, 24), (32, 12), "strong"),
    (["--global-nx", "64", "--global-ny", "32"], (64, 32), (64, 16), "strong"),   # config-3 style: an explicit global domain
])
def test_bench_launches_its_own_ranks(gpu, extra, glob, local, scaling):
    """`python bench.py --gpus 2` under no launcher: two rank processes (here sharing the one device, host-staged
    exchange), one JSON line from rank 0, the requested decomposition (2 ranks -> 1 x 2, src/pprts_base.F90:757-763)."""
    env = {k: "" for k in ()}
    clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + extra + SMALL, capture_output=True,
                       text=True, timeout=900, env=clean, cwd=ROOT)
    out = _line(p)
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["config"]["process_grid"] == "1x2"
    assert f"{glob[0]}x{glob[1]}x16 cells global ({local[0]}x{local[1]}x16 on rank 0)" in out["config"]["workload"]
    assert out["config"]["reason"] in (2, 3) and out["value"] > 0


def test_bench_eight_ranks_on_the_two_by_four_grid(gpu):
    """`python bench.py --gpus 8` on a 1-GPU box: config 3's 2 x 4 process grid (src/pprts_base.F90:757-763), here on a
    64 x 64 x 16 domain with the host-staged transport; fixed total work by default at N > 1 (BASELINE's metric reads
    "256x256x64 at 1/2/4/8 GPU")."""
    clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--global-nx", "64", "--global-ny", "64",
                        "--transport", "host", "--full"] + SMALL, capture_output=True, text=True, timeout=1200, env=clean, cwd=ROOT)
    out = _line(p)
    assert out["n_gpus"] == 8 and out["config"]["process_grid"] == "2x4" and out["scaling"] == "strong"
    assert "64x64x16 cells global (32x16x16 on rank 0)" in out["config"]["workload"]
    assert out["config"]["reason"] in (2, 3) and out["value"] > 0
    # the default at N > 1 is the metric's reading: the same global domain whatever N
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--nx", "32", "--ny", "24"] + SMALL,
                       capture_output=True, text=True, timeout=900, env=clean, cwd=ROOT)
    out = _line(p)
    assert out["scaling"] == "strong" and "32x24x16 cells global (32x12x16 on rank 0)" in out["config"]["workload"]


def test_bench_refuses_a_rank_count_mismatch(gpu):
    p = _run(["--gpus", "2"] + SMALL, env={"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)


def test_bench_survives_a_peer_transport_that_fails_during_the_solves(gpu):
    """Failure injection: the peer transport is attached (`--transport peer`: no self test) with a wait bound of a microsecond, so
    the first message between the two rank processes 'is lost'.  Every rank must leave the timed loop (bounded waits, fail-fast
    after the first expiry), agree on the failure, give the transport up -- including the preconditioner-halo agreement that one
    rank may already have cached over it -- and measure over the host-staged exchanges instead: one valid line."""
    clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    clean["TSX_PEER_TIMEOUT_S"] = "0.000001"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--transport", "peer", "--nx", "64", "--ny", "48"]
                       + SMALL, capture_output=True, text=True, timeout=600, env=clean, cwd=ROOT)
    out = _line(p)
    assert "falling back" in p.stderr
    assert out["config"]["transport"].startswith("host-staged") and "after the peer transport failed" in out["config"]["transport"]
    assert out["config"]["reason"] in (2, 3) and out["value"] > 0
    # same iteration count as the run that never touched the peer transport
    ref = _line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--transport", "host", "--nx", "64",
                                "--ny", "48"] + SMALL, capture_output=True, text=True, timeout=600, env=clean, cwd=ROOT))
    assert out["config"]["iterations"] == ref["config"]["iterations"]
