"""bench.py's host-side plumbing, without a GPU: the timed rounds, --dump-outputs and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("pool,warmup,steps", [(23, 3, 20), (5, 3, 20), (1, 0, 4), (4, 4, 4), (2, 3, 1)])
def test_rounds_run_every_step_once_on_its_own_fresh_input(pool, warmup, steps):
    total = warmup + steps
    slots = list(range(pool))   # slot s % pool holds step s's input, generated ahead
    held = list(range(pool))
    ran, regenerated = [], []

    def regen(s):
        slots[s % pool] = s
        regenerated.append(s)

    def step(i):
        assert slots[i % pool] == i, f"step {i} found {slots[i % pool]!r}"
        slots[i % pool] = "factored"
        ran.append(i)

    bench.run_rounds(0, warmup, pool, held, regen, step, lambda: None)
    dt = bench.run_rounds(warmup, steps, pool, held, regen, step, lambda: None)
    assert ran == list(range(total)) and dt >= 0.0
    assert (regenerated == []) == (pool >= total)   # inputs that fit are all generated before any clock starts


def test_dump_outputs_are_seeded_typed_and_within_64_mb(tmp_path):
    n = 300
    LU = torch.randn(n, n, dtype=torch.float64)
    ipiv, info = torch.arange(n, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "a"), torch, LU, ipiv, info)
    bench.dump_outputs(str(tmp_path / "b"), torch, LU, ipiv, info)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["info.npy", "ipiv.npy", "lu_diag.npy", "lu_sample.npy"]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "lu_diag.npy"), LU.diagonal().numpy())
    assert np.isin(np.load(tmp_path / "a" / "lu_sample.npy"), LU.numpy()).all()
    bench.dump_outputs(str(tmp_path / "c"), torch, LU.float(), ipiv, info)
    assert np.load(tmp_path / "c" / "lu_sample.npy").dtype == np.float32
    # the 8192^2 fp64 headline: sample + diag(U) + ipiv + info
    assert bench.DUMP_SAMPLE * 8 + 3 * 8192 * 8 + 8 <= 64 * 2 ** 20


def test_command_line_has_full_and_dump_outputs_and_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
