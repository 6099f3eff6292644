#!/usr/bin/env python3
"""
Times Context.lag_covariance (vgpa_lag_covariance) behind a free_energy on the two flagship contexts:

  l96   Lorenz-96, D = 40, RK4, Np = 1001, B = 512:     one anchor at 0 with stride 10; 8 anchors spread evenly, stride 10
  l63   Lorenz-63, RK4, Np = 1001, B = 65 536:          one anchor at 0 with stride 10

Device events on the context's stream around the call (StreamTimer of tools/bench_problem_batch.py, as its --mode theta), the median of
`--rounds` rounds x `--steps` calls.  Per case three times and two yardsticks:
  call_ms        the whole entry point: starting matrices, recursion, and the copy of the result to the host
  recursion_ms   the same call with stride = Np - 1 (two kept rows): the recursion without its output
  propagator_ms  the whole call of the propagator kind (same work, I for S_s)
  fwd_ms         the forward stepper of the same context in the same process: the fwd phase of the context's own profile events over free_energy
                 (the kernel vgpa_solve_fwd launches; `--mode forward` runs only that, for rocprofv3 --kernel-trace --stats in a run of its own)
  hbm_write_ms   the bytes the call must write over 6.3 TB/s (the copy rate a MI355X reaches), and host_copy_gbs: what the copy to the host got

    python tools/bench_lag_covariance.py [--cases l96,l63] [--rounds 3] [--steps 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_lag_covariance.py --mode forward --cases l96
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_COPY_TBS = 6.3
CONTEXTS = {"l96": dict(name="L96", d=40, n_pts=1001, dt=0.01, batch=512, anchor_sets={"anchor_0": [0], "anchors_8": list(range(0, 1001, 125))[:8]}),
            "l63": dict(name="L63", d=3, n_pts=1001, dt=0.01, batch=65536, anchor_sets={"anchor_0": [0]})}
STRIDE = 10


def context_with_state(cfg, batch):
    from bench_problem_batch import make_contexts
    ctxs, x0 = make_contexts(cfg["name"], cfg["d"], cfg["n_pts"], cfg["dt"], batch, modes=("shared",))
    c = ctxs["shared"]
    len_x = x0.shape[1]
    rng = np.random.default_rng(1)
    rows = x0[np.arange(min(64, batch)) % x0.shape[0]] + 0.05 * rng.standard_normal((min(64, batch), len_x))
    xb = c.alloc(batch * len_x)
    for i0 in range(0, batch, 64):
        xb.upload_at(i0 * len_x, rows[:min(64, batch - i0)])
    return c, xb


def raw_call(c, kind, anchors, stride, out):
    a = np.ascontiguousarray(anchors, dtype=np.int64)
    c._check(c._lib.vgpa_lag_covariance(c._h, kind, None, int(a.size), a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(stride),
                                        out.ctypes.data_as(ctypes.c_void_p)))


def run_case(key, rounds, steps, batch=None):
    from bench_problem_batch import StreamTimer
    cfg = CONTEXTS[key]
    B, d, n = batch or cfg["batch"], cfg["d"], cfg["n_pts"]
    c, xb = context_with_state(cfg, B)
    tm = StreamTimer(c)
    out = {"context": key, "model": cfg["name"], "D": d, "Np": n, "B": B, "method": "rk4", "stride": STRIDE}
    gb = c.alloc(xb.count)
    for _ in range(2):                                                              # warm-up (first-use allocations)
        c.sweep_enqueue(xb, gb)
        c.fetch_f()
    c.profile_begin()                                                               # (the phase events close behind a gradient: whole sweeps)
    for _ in range(steps):
        c.sweep_enqueue(xb, gb)
        f = c.fetch_f()
    pr = c.profile_end()
    assert np.all(np.isfinite(f))
    out["fwd_ms"] = round(pr["fwd_ms"] / (pr["n_sweeps"] / B), 4)                   # (the profile counts problems)
    gb.free()
    c.free_energy_dev(xb)
    n_keep = (n - 1) // STRIDE + 1
    for tag, anchors in cfg["anchor_sets"].items():
        na = len(anchors)
        full, tiny = np.empty((B, na, n_keep, d, d)), np.empty((B, na, 2, d, d))
        calls = {"call_ms": lambda: raw_call(c, 0, anchors, STRIDE, full), "recursion_ms": lambda: raw_call(c, 0, anchors, n - 1, tiny),
                 "propagator_ms": lambda: raw_call(c, 1, anchors, STRIDE, full)}
        ms = {k: [] for k in calls}
        for k, fn in calls.items():
            fn()                                                                    # warm-up (first-use allocations, page faults of `full`)
        for _ in range(rounds):
            for k, fn in calls.items():
                ms[k].append(float(np.median([tm.ms(fn) for _ in range(steps)])))
        assert np.all(np.isfinite(full[0])) and not np.any(full[0, -1, :(anchors[-1] + STRIDE - 1) // STRIDE])
        rec = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        rec["rounds_ms"] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
        nbytes = full.size * 8
        rec["bytes_written"] = nbytes
        rec["hbm_write_ms"] = round(nbytes / (HBM_COPY_TBS * 1e12) * 1e3, 4)
        rec["host_copy_gbs"] = round(nbytes / 1e9 / max((rec["call_ms"] - rec["recursion_ms"]) * 1e-3, 1e-9), 2)
        rec["recursion_over_fwd"] = round(rec["recursion_ms"] / out["fwd_ms"], 3)
        out[tag] = rec
    tm.close()
    c.close()
    return out


def run_forward(key, steps, batch=None):
    cfg = CONTEXTS[key]
    B = batch or cfg["batch"]
    c, xb = context_with_state(cfg, B)
    for _ in range(steps):
        f = c.free_energy_dev(xb)
    assert np.all(np.isfinite(f))
    c.close()
    return {"context": key, "B": B, "free_energy_calls": steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("lag", "forward"), default="lag")
    ap.add_argument("--cases", default="l96,l63")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="another batch size (smoke runs)")
    args = ap.parse_args()
    for key in args.cases.split(","):
        res = run_case(key, args.rounds, args.steps, args.batch) if args.mode == "lag" else run_forward(key, args.steps, args.batch)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
