"""bench.py's real N-rank body on the test box's one GPU (the N>1 path had only run up
to the launch).  ``--dist-backend gloo`` is the labelled oversubscribed rehearsal: both ranks run
the full body - calibration broadcast and its check on every rank, per-rank frame generation,
parity against the oracle before and after the timed region, the barrier-bracketed timed region,
the max-over-ranks time and the summed mismatch count - on device local_rank % device_count.
The driver's 8-GPU run uses the same body with backend "nccl" (RCCL), one rank per GPU."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("n,config", [(2, "c2"), (3, "c4")])
def test_bench_n_ranks_oversubscribed(n, config):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dist-backend",
                        "gloo", "--config", config, "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline",
                        "--no-dropin"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 20 and d["warmup"] == 5
    assert d["parity"]["frames_checked"] == n
    assert d["parity"]["mismatches"] == 0 and d["parity"]["mismatches_after_timed_region"] == 0
    sh = d["sharding"]
    assert sh["disjoint_and_complete"] and sh["global_frames"] == n * sh["frames_per_rank"]
    assert sh["calibration_broadcast"] == "verified on every rank"
    assert d["oversubscribed"]["ranks"] == n and "OVERSUBSCRIBED" in d["config"]["parallelism"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert "e2e_host" in d and d["e2e_host"]["value"] > 0


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _one_line(p):
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_rccl_branch_one_rank_under_torchrun():
    """the RCCL branch of bench.py (nccl process group, calibration broadcast on
    the device, all_reduce of times and counts, all_gather_object of frame indices) on hardware,
    launched as the driver launches N ranks - here N = 1."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--dist-backend", "nccl", "--steps", "20", "--warmup", "5", "--full",
                        "--no-cpu-baseline",
                        "--no-dropin", "--no-e2e", "--no-volume-roofline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    d = _one_line(p)
    sh = d["sharding"]
    assert "RCCL" in sh["backend"] and "1-rank process group" in sh["backend"], sh
    assert sh["calibration_broadcast"] == "verified on every rank" and sh["disjoint_and_complete"]
    assert d["parity"]["mismatches"] == 0 and d["n_gpus"] == 1 and d["value"] > 0


def test_bench_default_n1_dropin_and_unsettled():
    """The driver's N = 1 form (no torch.distributed environment): a one-rank RCCL group is created,
    and the line carries the drop-in pipeline figures (C2 / C4 at the reference defaults, parity 0)
    and the unsettled K-step figure."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20",
                        "--warmup", "5", "--full", "--no-cpu-baseline", "--no-e2e", "--no-volume-roofline",
                        "--no-batched"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    d = _one_line(p)
    assert "1-rank process group" in d["sharding"]["backend"]
    for c in ("c2", "c4"):
        r = d["dropin"][c]
        assert r["parity"]["mismatches"] == 0, r
        assert r["value"] > 0 and r["post_processing_ms"] > 0
        for k in ("bm_pass_left", "speckle_tile", "post_tail"):
            assert k in r["kernels_ms"], r["kernels_ms"]
    assert d["unsettled"]["value"] > 0


def test_bench_plain_run_is_lean_and_dumps_last_step(tmp_path):
    """Without --full the line carries the headline only (no parity, secondaries, roofline or CPU
    baseline), --steps sets the timed steps, and --dump-outputs writes the last timed step's maps:
    step K - 1 computes resident frame (K - 1) mod 4 of rank 0 (seed 1234 + index), bit-exact
    against the C oracle."""
    import numpy as np

    from depthestimation_amd.configs import CONFIGS, matcher_kwargs
    from depthestimation_amd.synthetic import stereo_pair
    from oracle.cref import CRef
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    steps = 7
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c4",
                        "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    d = _one_line(p)
    assert d["steps"] == steps and d["warmup"] == 2 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    cfg = CONFIGS["c4"]
    assert abs(d["value"] - cfg["H"] * cfg["W"] / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    assert d["parity"] is None and d["roofline"] is None and d["unsettled"] is None
    for k in ("cpu_baseline", "e2e_host", "dropin", "video_c4", "batched", "roofline_volume", "post_processing"):
        assert k not in d, k
    L, R, _ = stereo_pair(cfg["H"], cfg["W"], 0, cfg["num_disp"], seed=1234 + (steps - 1) % 4)
    want = CRef()(L, R, nthreads=16, **matcher_kwargs(cfg))
    fixed, flt = np.load(out / "disp_fixed.npy"), np.load(out / "disp_float.npy")
    assert fixed.dtype == np.float32 and flt.dtype == np.float32
    assert fixed.shape == flt.shape == (1, cfg["H"], cfg["W"])
    assert np.array_equal(fixed[0], want["fixed"].astype(np.float32))
    assert np.array_equal(flt[0], want["disp"])
