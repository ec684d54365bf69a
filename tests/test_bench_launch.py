"""bench.py as the driver may start it: `python bench.py --gpus N` with no launcher around it.

The parent process must bring up N ranks itself (a torch.distributed.run child, started before the parent touches the GPU)
or fail non-zero - never measure one GPU and print `n_gpus: 1`.  Covered here on the CPU over gloo with `--launch-check`
(rendezvous + rank count through the collective, nothing else); the measuring path needs GPUs (the GPU test at the end
runs it with --dump-outputs).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=300)


def test_self_launch_two_ranks_over_gloo():
    r = _run(["--gpus", "2", "--launch-check"], VPC_DIST_BACKEND="gloo")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world_size_env"] == 2 and out["backend"] == "gloo"


def test_refuses_to_measure_fewer_gpus_than_asked():
    import torch
    if torch.cuda.device_count() >= 64:
        return
    r = _run(["--gpus", "64", "--launch-check"])  # no rehearsal backend: 64 GPUs are not there
    assert r.returncode != 0
    assert "refusing" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--launch-check"], WORLD_SIZE="1", RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_dump_outputs_are_the_same_in_every_run(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs, as float32 .npy files, bit-equal in two runs with the same
    arguments (the settle steps a run needs do not change what the timed steps compute); --steps sets the timed steps."""
    names = ("loss_terms", "grad", "params", "exp_avg", "exp_avg_sq")
    outs = []
    for k in range(2):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / str(k))])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and "extra_configs" not in out
        outs.append({n: np.load(tmp_path / str(k) / f"{n}.npy") for n in names})
    for n in names:
        a = outs[0][n]
        assert a.dtype == np.float32 and a.size and np.all(np.isfinite(a)), n
        assert np.array_equal(a, outs[1][n]), n
