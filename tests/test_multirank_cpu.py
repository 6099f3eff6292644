"""CPU suite: the N > 1 plumbing (problem sharding, objective gather, max-over-ranks timing) with gloo, world size 2."""
import os
import sys
import socket

import numpy as np
import pytest

from conftest import ROOT, load_golden
from vgpa_amd.parallel import shard_range


def test_shard_range_partitions_exactly():
    for n in (0, 1, 5, 256, 257, 1001):
        for world in (1, 2, 3, 8):
            covered = []
            for r in range(world):
                lo, hi = shard_range(n, r, world)
                assert 0 <= lo <= hi <= n
                covered.extend(range(lo, hi))
            assert covered == list(range(n))
            sizes = [shard_range(n, r, world)[1] - shard_range(n, r, world)[0] for r in range(world)]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(4, 2, 2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, n_problems, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from vgpa_amd import parallel as par
    from oracle import vgpa_oracle as vo
    r, w = par.init_from_env("gloo")
    assert (r, w) == (rank, world)
    z = load_golden("ou_rk4_p")
    prob = vo.Problem.from_fixture(z)
    lo, hi = par.shard_range(n_problems, rank, world)
    # the objective of this rank's problems (the oracle stands in for the GPU sweep on this CPU-only test)
    f_local = [vo.free_energy(prob, z["x"] + 0.01 * i)[0] for i in range(lo, hi)]
    f_all = par.gather_objective(f_local, n_problems)
    t = par.max_over_ranks(1.0 + rank)
    par.barrier()
    np.save(os.path.join(out_dir, f"f_{rank}.npy"), f_all)
    np.save(os.path.join(out_dir, f"t_{rank}.npy"), np.array([t]))
    dist.destroy_process_group()


def test_two_rank_gloo_gather_and_timing(tmp_path):
    import torch.multiprocessing as mp
    world, n_problems = 2, 5
    mp.spawn(_worker, args=(world, _free_port(), n_problems, str(tmp_path)), nprocs=world, join=True)
    from oracle import vgpa_oracle as vo
    z = load_golden("ou_rk4_p")
    prob = vo.Problem.from_fixture(z)
    serial = np.array([vo.free_energy(prob, z["x"] + 0.01 * i)[0] for i in range(n_problems)])
    for rank in range(world):
        f_all = np.load(tmp_path / f"f_{rank}.npy")
        assert np.array_equal(f_all, serial)              # same problems, same order, on every rank
        assert float(np.load(tmp_path / f"t_{rank}.npy")[0]) == 2.0   # MAX over ranks of (1 + rank)


def _gather_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from vgpa_amd import parallel as par
    from vgpa_amd.numerics import OdeSolver
    par.init_from_env("gloo")
    n_pts, d = 7, 3                                    # slices of unequal length: 4 + 3 grid points

    class _Arr:                                        # what NativeShardedRecursion hands back: something with .numpy()
        def __init__(self, a):
            self.a = a

        def numpy(self):
            return self.a

    class _Rec:
        D, world = d, 2
        time_slice = (0, 4) if rank == 0 else (4, 7)

    lo, hi = _Rec.time_slice
    full_v = np.arange(n_pts * d, dtype=float).reshape(n_pts, d)
    full_m = np.arange(n_pts * d * d, dtype=float).reshape(n_pts, d, d) * 0.5
    v, m = OdeSolver._gather_time(_Rec, _Arr(full_v[lo:hi].copy()), _Arr(full_m[lo:hi].copy()), n_pts)
    assert np.array_equal(v, full_v) and np.array_equal(m, full_m)
    # D not a multiple of the world size: no sharded recursion (every rank steps by itself on its own GPU)
    assert OdeSolver.__new__(OdeSolver)._large(65, 4) is None
    par.barrier()
    open(os.path.join(out_dir, f"ok_{rank}"), "w").write("ok")
    dist.destroy_process_group()


def test_time_sharded_results_are_gathered_without_pickling(tmp_path):
    """OdeSolver under a process group (D > 64): the native driver's time-sharded (vector, matrix) slices come back as the whole grid
    on every rank through two tensor all-gathers (slices of unequal length padded); gloo, world size 2, a stand-in for the driver."""
    import torch.multiprocessing as mp
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok_0").exists() and (tmp_path / "ok_1").exists()


def _bench(args, env_extra, timeout=300):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_starts_its_own_ranks_when_no_launcher_is_around():
    """`python bench.py --gpus N` exactly as the driver types it (no torchrun, WORLD_SIZE unset): the script starts N ranks itself
    (torch.distributed.run as a CHILD of a process that has made no GPU call), they rendezvous, and `n_gpus` is N -- never a silent
    one-GPU run.  VGPA_BENCH_LAUNCH_ONLY=1 stops each rank after the rendezvous: no GPU in this container."""
    import json
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full"], {"VGPA_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    c5 = out.pop("config5")
    assert out == {"launcher": "ok", "n_gpus": 2, "ranks_seen": 2}
    assert "starting 2 ranks" in r.stderr
    # N > 1: the config-5 block runs in child processes of the ranks, with a process group of their own on a neighbouring port
    assert c5["child"] == "ok" and c5["ranks_seen"] == 2


def test_a_failing_config5_child_cannot_take_the_headline_line_with_it():
    """The D = 4096 block is the only part of the bench that puts several ranks through RCCL, which no one-GPU box can rehearse:
    at N > 1 it runs in child processes that the ranks start before they touch the GPU.  Children that hang are killed at
    --config5-timeout and the block reports it; the ranks go on and print their line, exit code 0."""
    import json
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full", "--config5-timeout", "5"],
               {"VGPA_BENCH_LAUNCH_ONLY": "1", "VGPA_BENCH_C5_TEST_HANG": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["ranks_seen"] == 2 and "did not finish" in out["config5"]["error"]
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full", "--no-config5"], {"VGPA_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode == 0 and json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["config5"] is None


def test_bench_refuses_a_world_size_that_disagrees_with_gpus():
    r = _bench(["--gpus", "2"], {"VGPA_BENCH_LAUNCH_ONLY": "1", "WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    r = _bench(["--gpus", "1"], {"VGPA_BENCH_LAUNCH_ONLY": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
    r = _bench(["--gpus", "0"], {})
    assert r.returncode != 0


def test_config5_default_grid_gives_every_rank_the_same_number_of_grid_points():
    """The strong-scaling block's time-parallel phases (energy terms, gradient: ~ 1/3 of the one-GPU time) scale with the LARGEST
    time slice.  The default grid of `bench.py --config5-np` must therefore split evenly over 1, 2, 4 and 8 ranks (VERDICT r3:
    Np = 9 gave rank 0 two grid points and the others one at N = 8).  vgpa_time_slice is the library's own ownership rule."""
    import ctypes
    import importlib.util
    import vgpa_amd as va
    spec = importlib.util.spec_from_file_location("bench_for_defaults", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        n = bench.parse().config5_np
    finally:
        sys.argv = argv
    lib = va.load()
    for world in (1, 2, 4, 8):
        sizes, covered = [], []
        for rank in range(world):
            lo, hi = ctypes.c_int(), ctypes.c_int()
            assert lib.vgpa_time_slice(n, rank, world, ctypes.byref(lo), ctypes.byref(hi)) == 0
            sizes.append(hi.value - lo.value)
            covered.extend(range(lo.value, hi.value))
        assert covered == list(range(n))
        assert max(sizes) == min(sizes) == n // world, (world, sizes)
    lo, hi = ctypes.c_int(), ctypes.c_int()
    assert lib.vgpa_time_slice(9, 0, 8, ctypes.byref(lo), ctypes.byref(hi)) == 0 and hi.value - lo.value == 2    # the old default
    assert lib.vgpa_time_slice(n, 8, 8, ctypes.byref(lo), ctypes.byref(hi)) == -1
