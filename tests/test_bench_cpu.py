"""CPU suite: the parts of bench.py that need no GPU -- the plain / --full split, the batch inputs and --dump-outputs."""
import os
import sys
import json
import subprocess
import importlib.util

import numpy as np

from conftest import ROOT


def _bench(args, env_extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=timeout)


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_for_cpu_tests", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_a_plain_run_starts_no_secondary_block():
    """Without --full the N > 1 launcher starts no config-5 child processes (with --full it does: test_multirank_cpu)."""
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"VGPA_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out == {"launcher": "ok", "n_gpus": 2, "ranks_seen": 2, "config5": None}


def test_dump_outputs_needs_a_timed_step():
    r = _bench(["--steps", "0", "--dump-outputs", "unused"], {})
    assert r.returncode != 0 and "--steps >= 1" in r.stderr


def test_batch_inputs_are_the_serial_ones_bit_for_bit():
    bench = _load_bench()
    x0 = np.random.default_rng(5).standard_normal(1003)
    for lo, world in ((0, 1), (7, 2)):
        got = bench.batch_inputs(x0, lo, 9, world)
        for i in range(9):
            gi = lo + i
            r = np.random.default_rng(0) if gi == 0 else np.random.default_rng(1000 + gi)
            want = x0 + 0.05 * r.standard_normal(x0.size)
            assert np.array_equal(got[i].view(np.int64), want.view(np.int64)), (lo, i)


class _FakeDeviceBuffer:
    """The one DeviceBuffer method dump_outputs uses, over a host array."""

    def __init__(self, a):
        self.a = a

    def download_at(self, offset, count):
        return self.a[offset:offset + count].copy()


def test_dump_outputs_writes_the_last_step_as_float64_files(tmp_path):
    bench = _load_bench()
    B, len_x = 40, 3000
    g = np.random.default_rng(3).standard_normal(B * len_x)
    f = np.random.default_rng(4).standard_normal(B)
    bench.dump_outputs(str(tmp_path / "a"), f, _FakeDeviceBuffer(g), B, len_x)
    bench.dump_outputs(str(tmp_path / "b"), f, _FakeDeviceBuffer(g), B, len_x)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["F.npy", "grad0.npy", "grad_index.npy", "grad_problems.npy", "grad_sample.npy"]
    arrays = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    assert np.array_equal(arrays["F"], f) and np.array_equal(arrays["grad0"], g[:len_x])
    idx, probs = arrays["grad_index"].astype(np.int64), arrays["grad_problems"].astype(np.int64)
    assert idx.size == len_x and probs.size == bench.DUMP_PROBLEMS and np.all(np.diff(probs) > 0)
    assert np.array_equal(arrays["grad_sample"], g.reshape(B, len_x)[probs][:, idx])
    for n in names:                                          # the sample is fixed: two dumps of the same outputs are identical
        assert np.array_equal(np.load(tmp_path / "b" / n), arrays[n[:-4]]), n
