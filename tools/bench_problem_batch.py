"""
Throughput of a batch of independent datasets (Context.set_problem_data) or parameter points (Context.set_problem_params)
against the shared batch, one JSON line.

Two configurations, each in four contexts alive in one process: "shared" (every problem on the dataset of vgpa_config), "data"
(per-problem observation values, m0, S0, e0), "data_t" (the same plus per-problem observation times) and "params" (the shared
dataset at per-problem theta and Sigma = sigma_p^2 I, Context.set_problem_params).  The modes alternate
round by round; each round times `--steps` sweeps of one mode with the context's phase events (device time of the fused sweep,
vgpa_profile_begin / _end), and the median per round is reported.

    python tools/bench_problem_batch.py [--rounds 5] [--steps 10]
    python tools/bench_problem_batch.py --mode theta [--rounds 5] [--steps 10]
    python tools/bench_problem_batch.py --mode obs [--rounds 5] [--steps 10] [--variants shared,obs_model,obs_counts]

  l96   Lorenz-96, D = 40, RK4, Np = 1001, B = 512     (bench.py's headline configuration)
  l63   Lorenz-63, D = 3, RK4, Np = 1001, B = 65536    (bench.py's config2 block: the lane-per-problem kernels)

--mode obs: the cost of a per-problem observation model (Context.set_problem_obs_model), timed like the default mode, in three
contexts: "shared" (the model of vgpa_config), "obs_model" (per-problem R_p = R (1 + 0.1 (p mod 4)) and H_p, a 0/1 mask that drops
component i when (i + p) mod 3 = 0; equal counts) and "obs_counts" (the same with per-problem counts cycling through M, M - 1, 1).
All three on the dataset of vgpa_config, so that the difference is the observation model alone.  --variants picks a subset (the shared one alone also runs on a library without the entry point).

--mode theta: the time of Context.theta_gradient() behind a free_energy, beside the time of that free_energy, on the same contexts
(and on one more: l96_ld, Lorenz-96, D = 1024, RK4, Np = 33, B = 1).  Both are timed with a pair of device events on the context's
stream around the call (each call ends with its own synchronisation: F, resp. the B n_theta results, come back to the host).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def datasets(name, d, n_pts, dt, nset, seed0):
    from helpers import build_problem
    return [build_problem(name, "RK4", (n_pts - 1) * dt, dt, d, seed=seed0 + j) for j in range(nset)]


def make_contexts(name, d, n_pts, dt, B, nset=4, modes=("shared", "data", "data_t", "params")):
    import vgpa_amd as va
    from helpers import SEED
    ps = datasets(name, d, n_pts, dt, nset, SEED)
    p0 = ps[0]
    theta = p0["model"].theta
    e0 = float(p0["kl0"](p0["m0"], p0["s0"]))
    kw = dict(sigma=p0["model"].sigma, theta=theta, m0=p0["m0"], s0=p0["s0"], obs_t=p0["obs_t"], obs_y=p0["obs_y"],
              obs_noise=p0["obs_noise"], e0=e0, batch=B)
    m = len(p0["obs_t"])
    j = np.arange(B) % nset
    obs_y = np.stack([np.reshape(ps[i]["obs_y"], (m, d)) for i in j])
    m0 = np.stack([np.asarray(ps[i]["m0"], dtype=float) + 0.01 * (k % 97) for k, i in enumerate(j)])
    s0 = np.stack([np.asarray(ps[i]["s0"], dtype=float) for i in j])
    e0s = np.array([float(ps[i]["kl0"](m0[k], s0[k])) for k, i in enumerate(j)])
    obs_t = np.stack([np.minimum(np.asarray(p0["obs_t"], dtype=np.int64) + (i % 3), n_pts - 1) for i in j])
    k = np.arange(B)
    th = np.atleast_1d(np.asarray(theta, dtype=float))[None, :] * (1.0 + 0.05 * (k % 5))[:, None]
    sig = np.asarray(p0["model"].sigma, dtype=float)[None] * (1.0 + 0.1 * (k % 4))[:, None, None]      # sigma_p^2 I
    # per-problem observation models (--mode obs)
    r0 = np.reshape(np.asarray(p0["obs_noise"], dtype=float), (d, d))
    obs_r = r0[None] * (1.0 + 0.1 * (k % 4))[:, None, None]
    obs_h = np.stack([np.diag(((np.arange(d) + p) % 3 != 0).astype(float)) for p in range(B)]) if d > 1 else None
    counts = np.array([(m, m - 1, 1)[p % 3] for p in range(B)], dtype=np.int32)
    ctxs = {}
    for mode in modes:
        c = va.Context(name, "RK4", d, n_pts, dt, **kw)
        if mode in ("obs_model", "obs_counts"):
            c.set_problem_obs_model(n_obs=counts if mode == "obs_counts" else None, obs_noise=obs_r, obs_h=obs_h)
        if mode in ("data", "data_t"):
            c.set_problem_data(obs_t=obs_t if mode == "data_t" else None, obs_y=obs_y, m0=m0, s0=s0, e0=e0s)
        if mode == "params":
            c.set_problem_params(theta=th, sigma=sig)
        ctxs[mode] = c
    x0 = np.stack([ps[i]["vgp"].initialization() for i in range(nset)])
    return ctxs, x0


def run(name, d, n_pts, dt, B, rounds, steps, modes=("shared", "data", "data_t", "params")):
    ctxs, x0 = make_contexts(name, d, n_pts, dt, B, modes=modes)
    len_x = x0.shape[1]
    rng = np.random.default_rng(1)
    rows = x0[np.arange(64) % x0.shape[0]] + 0.05 * rng.standard_normal((64, len_x))
    bufs = {}
    for mode, c in ctxs.items():
        xb, gb = c.alloc(B * len_x), c.alloc(B * len_x)
        for i0 in range(0, B, 64):
            k = min(64, B - i0)
            xb.upload_at(i0 * len_x, rows[:k])
        bufs[mode] = (xb, gb)
        for _ in range(2):                       # warm-up (first-use allocations)
            c.sweep_enqueue(xb, gb)
            c.fetch_f()
    ms = {mode: [] for mode in ctxs}
    for _ in range(rounds):
        for mode, c in ctxs.items():
            xb, gb = bufs[mode]
            c.profile_begin()
            for _ in range(steps):
                c.sweep_enqueue(xb, gb)
                f = c.fetch_f()
            pr = c.profile_end()
            sweeps = pr["n_sweeps"] / B
            ms[mode].append((pr["fwd_ms"] + pr["energy_ms"] + pr["bwd_ms"] + pr["grad_ms"]) / sweeps)
            assert np.all(np.isfinite(f))
    for c in ctxs.values():
        c.close()
    med = {mode: float(np.median(v)) for mode, v in ms.items()}
    out = {"B": B, "D": d, "Np": n_pts,
           "ms_per_sweep": {m: round(v, 4) for m, v in med.items()},
           "sweeps_per_s": {m: round(B * 1e3 / v, 1) for m, v in med.items()}}
    if "shared" in med:
        out.update({"ratio_" + m: round(med["shared"] / v, 4) for m, v in med.items() if m != "shared"})
    out["rounds_ms"] = {m: [round(x, 4) for x in v] for m, v in ms.items()}
    return out


class StreamTimer(object):
    """Device time of what a call enqueues on a context's stream: two HIP events around it (the runtime the library brought in)."""

    def __init__(self, ctx):
        import ctypes
        hip = ctypes.CDLL(None)
        if not hasattr(hip, "hipEventCreate"):
            hip = ctypes.CDLL("libamdhip64.so")
        self.hip, self.ct = hip, ctypes
        self.stream = ctypes.c_void_p(ctx._lib.vgpa_stream(ctx._h))
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            assert hip.hipEventCreate(ctypes.byref(e)) == 0
        hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        hip.hipEventDestroy.argtypes = [ctypes.c_void_p]

    def ms(self, call):
        assert self.hip.hipEventRecord(self.ev[0], self.stream) == 0
        call()
        assert self.hip.hipEventRecord(self.ev[1], self.stream) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        out = self.ct.c_float()
        assert self.hip.hipEventElapsedTime(self.ct.byref(out), self.ev[0], self.ev[1]) == 0
        return float(out.value)

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def run_theta(name, d, n_pts, dt, B, rounds, steps, modes=("shared", "data", "data_t", "params"), nset=4):
    ctxs, x0 = make_contexts(name, d, n_pts, dt, B, nset=nset, modes=modes)
    len_x = x0.shape[1]
    rng = np.random.default_rng(1)
    rows = x0[np.arange(min(64, B)) % x0.shape[0]] + 0.05 * rng.standard_normal((min(64, B), len_x))
    bufs, timers = {}, {}
    for mode, c in ctxs.items():
        xb = c.alloc(B * len_x)
        for i0 in range(0, B, 64):
            xb.upload_at(i0 * len_x, rows[:min(64, B - i0)])
        bufs[mode], timers[mode] = xb, StreamTimer(c)
        for _ in range(2):                       # warm-up (first-use allocations)
            c.free_energy_dev(xb)
            g = c.theta_gradient()
        assert np.all(np.isfinite(g))
    ms = {mode: {"free_energy": [], "theta_gradient": []} for mode in ctxs}
    for _ in range(rounds):
        for mode, c in ctxs.items():
            xb, tm = bufs[mode], timers[mode]
            tf = [tm.ms(lambda: c.free_energy_dev(xb)) for _ in range(steps)]
            tg = [tm.ms(c.theta_gradient) for _ in range(steps)]
            ms[mode]["free_energy"].append(float(np.median(tf)))
            ms[mode]["theta_gradient"].append(float(np.median(tg)))
    for mode, c in ctxs.items():
        timers[mode].close()
        c.close()
    out = {"B": B, "D": d, "Np": n_pts}
    for mode, v in ms.items():
        out[mode] = {k: round(float(np.median(t)), 4) for k, t in v.items()}
        out[mode]["rounds_ms"] = {k: [round(x, 4) for x in t] for k, t in v.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("sweep", "theta", "obs"), default="sweep")
    ap.add_argument("--variants", default="shared,obs_model,obs_counts", help="--mode obs: the contexts to time")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--l63-batch", type=int, default=65536)
    args = ap.parse_args()
    if args.mode == "theta":
        out = {"tool": "bench_problem_batch", "mode": "theta", "unit": "ms per call (device events)",
               "l96": run_theta("L96", 40, 1001, 0.01, 512, args.rounds, args.steps),
               "l63": run_theta("L63", 3, 1001, 0.01, args.l63_batch, args.rounds, args.steps),
               "l96_ld": run_theta("L96", 1024, 33, 0.01, 1, args.rounds, args.steps, modes=("shared",), nset=1)}
        print(json.dumps(out), flush=True)
        return
    if args.mode == "obs":
        modes = tuple(v for v in args.variants.split(",") if v)
        out = {"tool": "bench_problem_batch", "mode": "obs",
               "l96": run("L96", 40, 1001, 0.01, 512, args.rounds, args.steps, modes=modes),
               "l63": run("L63", 3, 1001, 0.01, args.l63_batch, args.rounds, args.steps, modes=modes)}
        print(json.dumps(out), flush=True)
        return
    out = {"tool": "bench_problem_batch",
           "l96": run("L96", 40, 1001, 0.01, 512, args.rounds, args.steps),
           "l63": run("L63", 3, 1001, 0.01, args.l63_batch, args.rounds, args.steps)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
