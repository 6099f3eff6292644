"""
Time of Context.sample_paths (vgpa_sample_paths), Context.sample_paths_weighted (vgpa_sample_paths_weighted), Context.particle_filter
(vgpa_particle_filter), Context.particle_statistics (vgpa_particle_statistics), Context.particle_events (vgpa_particle_events), Context.particle_moments (vgpa_particle_moments),
Context.particle_covariance (vgpa_particle_covariance), Context.particle_marginals (vgpa_particle_marginals), Context.particle_paths (vgpa_particle_paths), Context.particle_backward_paths
(vgpa_particle_backward_paths), Context.particle_backward_moments (vgpa_particle_backward_moments) and Context.particle_forecast (vgpa_particle_forecast) on their jobs, one JSON line.

    python tools/bench_sample_paths.py [--rounds 3] [--calls 5] [--jobs a,b,c,aw,aw0,bw,bw0,af64_0,af64_5,af1024_0,af1024_5,bf64_0,...]
    python tools/bench_sample_paths.py --statistics [--filter-problems 4096]      # the as* and bs* jobs
    python tools/bench_sample_paths.py --events [--filter-problems 4096]          # the ae* and be* jobs
    python tools/bench_sample_paths.py --moments [--filter-problems 4096]         # the am* and bm* jobs
    python tools/bench_sample_paths.py --covariance [--filter-problems 4096]      # the ac* and bc* jobs
    python tools/bench_sample_paths.py --marginals [--filter-problems 4096] [--levels 31]      # the ah* and bh* jobs
    python tools/bench_sample_paths.py --paths [--filter-problems 4096] [--paths-strides 1,10]      # the ap* and bp* jobs, once per stride
    python tools/bench_sample_paths.py --backward-moments [--smooth-problems 8]      # the aw*, bw* and ow* jobs
    python tools/bench_sample_paths.py --backward [--filter-problems 4096] [--paths-strides 10] [--parent-json FILE]      # the ab* and bb* jobs
    python tools/bench_sample_paths.py --gibbs [--filter-problems 4096]           # the ag* and bg* jobs
    python tools/bench_sample_paths.py --lag-covariance [--lag-problems 512] [--filter-problems 4096]      # the al* and bl* jobs
    python tools/bench_sample_paths.py --forecast [--forecast-problems 512] [--forecast-particles 4096] [--forecast-horizon 1000]

  a   posterior kind, Lorenz-96, D = 40, Np = 1001, B = 512:   64 paths per problem, stride 100
  b   posterior kind, Lorenz-63, Np = 1001, B = 65536:          1 path per problem,  stride 100
  c   model kind on the context of b:                           1 path per problem,  stride 1
  aw, bw     the weighted twins of a and b: the same paths stored, and the two sums and x_0 of every path
  aw0, bw0   ... weights only: no path is stored or copied
  af<n>_<f>, bf<n>_<f>   the particle filter on the contexts of a and b: n = 64 or 1024 particles per problem, ess_fraction f = 0 (never
             resampled: the weights of aw0 / bw0, cut at the observations) or 5 (0.5), histories off; --filter-problems caps B of the
             b context's filter jobs (1024 particles on 65536 problems are 1.6 GB of final states to copy)

  as<n>_<f>, bs<n>_<f>   (--statistics selects all eight) particle_statistics with the arguments of af<n>_<f> / bf<n>_<f>, the mean reduced on
             the device and no rows copied, and particle_filter itself, the two calls alternating inside every round: both times and their
             ratio

  ae<n>, be<n>   (--events selects all four) particle_events on the contexts of a and b: n = 64 or 1024 particles per problem, ess_fraction 0.5,
             stride 1, the level of every component the mean of the filter's final particles, the sides alternating, the mean and the
             first-passage distribution reduced on the device and no rows copied; beside it particle_statistics (the same walk, the same
             number of carried values, the same gather) and particle_filter with the same arguments, the three calls alternating inside
             every round: the three times and the ratios

  am<n>_<s>, bm<n>_<s>   (--moments selects all twelve) particle_moments on the contexts of a and b: n = 64 or 1024 particles per problem,
             ess_fraction 0.5, every s-th grid index kept (s = 1, 10 or 1004: beyond the grid, index 0 alone is reduced -- the replay
             without its reductions), and particle_filter with the same arguments, the two calls alternating inside every round: both
             times, their ratio, the partial-sum buffer on the device and the result copied

  ac<n>_<s>, bc<n>_<s>   (--covariance selects all ten) particle_covariance on the contexts of a and b: n = 64 or 1024 particles per problem,
             ess_fraction 0.5, every s-th grid index kept -- s = 10 or 1004, and on the context of b also 1 (on a, D = 40, the partial
             sums of stride 1 take 3.5 GB at n = 64 and 56 GB at n = 1024, the matrices 6.6 GB to copy) --, and particle_moments and
             particle_filter with the same arguments, the three calls alternating inside every round: the three times, the ratios to
             particle_moments and to particle_filter, the partial-sum buffer on the device and the result copied

  ah<n>_<s>, bh<n>_<s>   (--marginals selects all eight) particle_marginals on the contexts of a and b: n = 64 or 1024 particles per problem,
             ess_fraction 0.5, every s-th grid index kept (s = 1 or 10), per problem and component the --levels levels of
             particles.gaussian_ladder over the cached posterior's m_t -+ 4 sqrt(S_t), and particle_moments with the same arguments -- the
             same filter, backward pass and replay, another reduction --, the two calls alternating inside every round: both times, their
             ratio and what each copies to the host

  ap<n>_<K>, bp<n>_<K>   (--paths selects all eight, each once per stride of --paths-strides) particle_paths on the contexts of a and b:
             n = 64 or 1024 particles per problem, ess_fraction 0.5, K = 16 or 64 trajectories per problem drawn from the final weights,
             and particle_filter with the same arguments, the two calls alternating inside every round: both times, their ratio, the
             trajectories copied and how many different paths the K trajectories have in the first and in the last stretch

  ab<n>_<K>, bb<n>_<K>   (--backward selects all eight, each once per stride of --paths-strides) particle_backward_paths with the arguments
             of ap<n>_<K> / bp<n>_<K>, and particle_paths and particle_filter with the same arguments, the three calls alternating inside
             every round: the three times, the ratios, and how many different paths the K trajectories have in every stretch (the median
             over the problems) under backward simulation and under the genealogy.  --parent-json: the output of the parent commit's
             `--paths` run of the same jobs and strides on the same box (its own checkout and library, its processes alternating with
             this tool's): its particle_paths time is reported beside, as parent_paths_ms_per_call

  ag<n>, bg<n>   (--gibbs selects all six) particle_conditional on the contexts of a and b: n = 16, 64 or 1024 particles per problem,
             ess_fraction 0.5, the reference the trajectory of particle_paths(n, seed 2, n_draw 1), and particle_paths (one trajectory,
             stride 1) and particle_filter with the same arguments, the three calls alternating inside every round: the three times,
             the ratios, the share of the grid on which the sweep left the reference and how often the pinned slot's sampled ancestor
             was another slot (from one more call with the histories, where they take at most 1 GiB on the host).  --parent-json: the
             output of this tool, copied into the parent commit's checkout and run there with `--gibbs` on the same box (that checkout
             has no particle_conditional: the job then times particle_filter and particle_paths alone), its processes alternating
             with this tree's: the parent's two times are reported beside, as parent_filter_ms_per_call / parent_paths_ms_per_call

  al1024, bl64   (--lag-covariance selects both) particle_lag_covariance on the contexts of a (1024 particles; --lag-problems caps its B) and
             b (64 particles; --filter-problems caps its B): ess_fraction 0.5, stride 10, 8 anchors at 0, 120, ... 840, and beside it the
             only way to the same numbers without it: particle_paths(n_draw = n_paths, slots = 0 .. n-1) with the same arguments and the
             contraction on the host (one BLAS product per problem and anchor), timed as one call with the host clock; the two alternate
             inside every round.  Both times, their ratio, what each copies, and the contraction's FLOP count 2 B n_anchor n_keep n D^2

  --forecast   particle_forecast from a given cloud on a bare Lorenz-96 context (a model, theta, Sigma and dt: nothing evaluated), D = 40,
             B = 512, n = 4096 equally weighted particles, H = 1000 steps, no members, once with stride H (the sums at h = 0 and H alone)
             and once with stride 1 (the sums at every step), and beside them the model-kind sampler on the same lanes -- sample_paths(
             "model", n, stride H, x0) on a grid of H + 1 points: the same steps without a reduction.  The three calls alternate inside
             every round; the excess of stride 1 over the sampler is what the reductions cost.  up_mb / d2h_mb: what each call copies.  (dt is
             a tenth of the other jobs': the explicit Euler step of Lorenz-96 at dt = 0.01 sends a few of 2 million noisy paths to
             infinity within 1000 steps, and the time of a step does not depend on dt)

The posterior jobs read the x a free_energy_dev left cached (x=None: nothing is uploaded); every job draws its start from (m0, S0).  A call
is timed with a pair of device events on the context's stream around it -- the host work of the call (the Cholesky factors), the kernel and
the copy of the result to the host; the median over the calls of a round, then the median over the rounds.  Beside each time:

  numpy_ms   the same job in the numpy restatement of tests/test_sample_paths_cpu.py on one host core, run on `--numpy-problems` problems
             and scaled linearly to B
  floor_ms   the bytes that must move in device memory -- x once per workgroup (a: one workgroup per 64 paths of a problem) or per lane
             (b), the stored points -- at the 8 TB/s DESIGN.md s.5 uses; d2h_mb is the result that travels to the host on top of it
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12
N_PTS, DT = 1001, 0.01
JOBS = {"a": ("L96", 40, 512, "posterior", 64, 100), "b": ("L63", 3, 65536, "posterior", 1, 100), "c": ("L63", 3, 65536, "model", 1, 1),
        "o": ("OU", 1, 65536, "posterior", 1, 100)}      # (o: the context of the ow* jobs alone)
WEIGHTED = {"aw": ("a", True), "aw0": ("a", False), "bw": ("b", True), "bw0": ("b", False)}      # job -> (its unweighted twin, paths stored)
FILTER = {f"{t}f{n}_{f}": (t, n, 0.1 * f) for t in "ab" for n in (64, 1024) for f in (0, 5)}      # job -> (context of, particles, ess_fraction)
STATS = {f"{t}s{n}_{f}": (t, n, 0.1 * f) for t in "ab" for n in (64, 1024) for f in (0, 5)}       # job -> as FILTER
EVENTS = {f"{t}e{n}": (t, n, 0.5) for t in "ab" for n in (64, 1024)}       # job -> as FILTER
MOMENTS = {f"{t}m{n}_{s}": (t, n, s) for t in "ab" for n in (64, 1024) for s in (1, 10, N_PTS + 3)}          # job -> (context of, particles, stride)
COV = {f"{t}c{n}_{s}": (t, n, s) for t in "ab" for n in (64, 1024) for s in (1, 10, N_PTS + 3) if t == "b" or s > 1}          # job -> as MOMENTS
MARG = {f"{t}h{n}_{s}": (t, n, s) for t in "ab" for n in (64, 1024) for s in (1, 10)}                       # job -> as MOMENTS
PATHS = {f"{t}p{n}_{k}": (t, n, k) for t in "ab" for n in (64, 1024) for k in (16, 64)}           # job -> (context of, particles, trajectories)
BACKWARD = {f"{t}b{n}_{k}": (t, n, k) for t in "ab" for n in (64, 1024) for k in (16, 64)}        # job -> as PATHS
# (--backward-moments selects all six) particle_backward_moments beside particle_moments (the genealogical call), particle_backward_paths with
# K = n (the existing kernel forming the same n^2 scores once, with its Gumbels) and particle_filter, the four calls alternating inside every
# round, on --smooth-problems problems of the contexts of a, b and o: the histories take B M n (D + 1) doubles
SMOOTH = {f"{t}w{n}": (t, n) for t in "abo" for n in (1024, 4096)}                                # job -> (context of, particles)
GIBBS = {f"{t}g{n}": (t, n) for t in "ab" for n in (16, 64, 1024)}                                # job -> (context of, particles)
LAG = {"al1024": ("a", 1024, 10), "bl64": ("b", 64, 10)}                                          # job -> as MOMENTS
LAG_ANCHORS = 8


def tree():
    """the commit of the measured tree: tools/stamp_tree.sh's file (the GPU box has no .git), VGPA_HEAD, or git itself"""
    path = os.path.join(ROOT, "vgpa_amd", "_tree.txt")
    if os.path.exists(path):
        with open(path) as fh:
            return fh.read().strip()
    if os.environ.get("VGPA_HEAD"):
        return os.environ["VGPA_HEAD"]
    try:
        import subprocess
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], text=True).strip()
    except Exception:
        return "unknown"


def numpy_ms(p0, x_row, d, kind, n_paths, stride, n_problems, B):
    from test_sample_paths_cpu import sample_paths_numpy
    m = p0["model"]
    q = types.SimpleNamespace(model=m._model_id, dim_d=d, n_pts=N_PTS, dt=DT, theta=m.theta, sigma=m.sigma, m0=p0["m0"], s0=p0["s0"])
    t0 = time.perf_counter()
    for k in range(n_problems):
        sample_paths_numpy(q, kind, x_row, None, n_paths, stride, 1, index=k)
    return (time.perf_counter() - t0) * 1e3 / n_problems * B


def run_forecast(B, n, horizon, rounds, calls):
    import vgpa_amd as va
    d = 40
    rng = np.random.default_rng(1)
    c = va.Context("L96", "euler", d, horizon + 1, 0.1 * DT, sigma=np.diag(3.0 + rng.random(d)), theta=[8.0], batch=B)
    from bench_problem_batch import StreamTimer
    tm = StreamTimer(c)
    x0 = 8.0 + rng.standard_normal((B, d))
    cloud = np.ascontiguousarray(x0[:, None, :] + 0.5 * rng.standard_normal((B, n, d)))
    calls_of = {"sampler": lambda: c.sample_paths("model", n, 1, stride=horizon, x0=x0),
                "forecast_stride_h": lambda: c.particle_forecast(horizon, seed=1, stride=horizon, cloud=cloud, index0=0),
                "forecast_stride_1": lambda: c.particle_forecast(horizon, seed=1, stride=1, cloud=cloud, index0=0)}
    res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
    far, near = res0["forecast_stride_h"], res0["forecast_stride_1"]
    assert res0["sampler"].shape == (B, n, 2, d) and np.all(np.isfinite(res0["sampler"]))
    assert near["moments"].shape == (B, horizon + 1, 2, d) and np.all(np.isfinite(near["moments"]))
    assert np.array_equal(far["state_end"], near["state_end"]) and np.array_equal(far["moments"], near["moments"][:, ::horizon])
    assert np.allclose(near["moments"][:, 0, 0], cloud.mean(axis=1), rtol=1e-12, atol=0.0)
    spread = float(np.median(np.sqrt(np.maximum(near["moments"][:, -1, 1] - near["moments"][:, -1, 0] ** 2, 0.0))))
    del res0, far, near
    per_round = {k: [] for k in calls_of}
    for _ in range(rounds):
        ms = {k: [] for k in calls_of}
        for _ in range(calls):
            for k, f in calls_of.items():
                ms[k].append(tm.ms(f))
        for k in calls_of:
            per_round[k].append(float(np.median(ms[k])))
    med = {k: float(np.median(v)) for k, v in per_round.items()}
    tm.close()
    c.close()
    out = {"job": "forecast", "model": "L96", "D": d, "B": B, "kind": "forecast", "n_paths": n, "horizon": horizon}
    for k in calls_of:
        out[k + "_ms_per_call"] = round(med[k], 3)
        out[k + "_rounds_ms"] = [round(v, 3) for v in per_round[k]]
    cloud_mb = 8.0 * B * n * d / 1e6
    out.update(stride_1_over_sampler=round(med["forecast_stride_1"] / med["sampler"], 4),
               stride_h_over_sampler=round(med["forecast_stride_h"] / med["sampler"], 4), median_spread_at_h=round(spread, 4),
               sampler_d2h_mb=round(2 * cloud_mb, 1), forecast_up_mb=round(cloud_mb, 1),
               forecast_stride_h_d2h_mb=round(cloud_mb + 8.0 * B * 2 * 2 * d / 1e6, 1),
               forecast_stride_1_d2h_mb=round(cloud_mb + 8.0 * B * (horizon + 1) * 2 * d / 1e6, 1),
               partial_buffer_stride_1_mb=round(8.0 * B * ((n + 63) // 64) * (horizon + 1) * 2 * d / 1e6, 1))
    return out


def run(job, rounds, calls, numpy_problems, cache, filter_problems=0, paths_stride=1, parent=None, n_levels=31, lag_problems=0, smooth_problems=8):
    from bench_problem_batch import StreamTimer, make_contexts
    twin, stored = WEIGHTED.get(job, (job, True))
    weighted = job in WEIGHTED
    if job in LAG:
        twin = LAG[job][0]
    elif job in FILTER or job in STATS or job in EVENTS or job in MOMENTS or job in COV or job in MARG or job in PATHS or job in BACKWARD or job in GIBBS:
        twin = (FILTER.get(job) or STATS.get(job) or EVENTS.get(job) or MOMENTS.get(job) or COV.get(job) or MARG.get(job) or PATHS.get(job) or BACKWARD.get(job) or GIBBS[job])[0]
    if job in SMOOTH:
        twin = SMOOTH[job][0]
    name, d, B, kind, n_paths, stride = JOBS[twin]
    if job in SMOOTH:
        B = min(B, smooth_problems)
    if (job in FILTER or job in STATS or job in EVENTS or job in MOMENTS or job in COV or job in MARG or job in PATHS or job in BACKWARD or job in GIBBS) and twin == "b" and filter_problems:
        B = min(B, filter_problems)
    if job in LAG:
        B = min(B, filter_problems if twin == "b" and filter_problems else B, lag_problems if twin == "a" and lag_problems else B)
    if (name, B) not in cache:                        # (b and c share a context)
        from helpers import SEED, build_problem
        ctxs, x0 = make_contexts(name, d, N_PTS, DT, B, modes=("shared",))
        c = ctxs["shared"]
        len_x = x0.shape[1]
        rows = x0[np.arange(64) % x0.shape[0]] + 0.05 * np.random.default_rng(1).standard_normal((64, len_x))
        xb = c.alloc(B * len_x)
        for i0 in range(0, B, 64):
            xb.upload_at(i0 * len_x, rows[:min(64, B - i0)])
        c.free_energy_dev(xb)
        cache[(name, B)] = (c, xb, rows[0], build_problem(name, "RK4", (N_PTS - 1) * DT, DT, d, seed=SEED), StreamTimer(c))
    c, xb, x_row, p0, tm = cache[(name, B)]
    len_x = N_PTS * d * (d + 1)
    n_keep = (N_PTS - 1) // stride + 1
    if job in STATS:
        _, n_paths, frac = STATS[job]
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=frac),
                    "statistics": lambda: c.particle_statistics(n_paths, 1, ess_fraction=frac)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        assert all(np.array_equal(res0["filter"][k], res0["statistics"][k]) for k in ("log_w", "state", "ess", "resampled"))
        assert res0["statistics"]["mean"].shape == (B, 3, d) and np.all(np.isfinite(res0["statistics"]["mean"]))
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "statistics", "n_paths": n_paths, "ess_fraction": frac,
                "statistics_ms_per_call": round(med["statistics"], 4), "filter_ms_per_call": round(med["filter"], 4),
                "ratio": round(med["statistics"] / med["filter"], 4),
                "statistics_rounds_ms": [round(v, 4) for v in per_round["statistics"]],
                "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
                "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + 3 * d) / 1e6, 1)}
    if job in EVENTS:
        _, n_paths, frac = EVENTS[job]
        flt0 = c.particle_filter(n_paths, 1, ess_fraction=frac)
        levels, side = flt0["state"].mean(axis=1), np.where(np.arange(d) % 2 == 0, 1, -1)
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=frac),
                    "statistics": lambda: c.particle_statistics(n_paths, 1, ess_fraction=frac),
                    "events": lambda: c.particle_events(n_paths, 1, levels, side=side, ess_fraction=frac)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        assert all(np.array_equal(res0["filter"][k], res0["events"][k]) for k in ("log_w", "state", "ess", "resampled"))
        ev = res0["events"]
        assert ev["mean"].shape == (B, 3, d) and ev["cdf"].shape == (B, N_PTS, d) and np.all(np.isfinite(ev["mean"])) and np.all(np.diff(ev["cdf"], axis=1) >= 0.0)
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "events", "n_paths": n_paths, "ess_fraction": frac, "stride": 1,
                "events_ms_per_call": round(med["events"], 4), "statistics_ms_per_call": round(med["statistics"], 4),
                "filter_ms_per_call": round(med["filter"], 4), "events_over_statistics": round(med["events"] / med["statistics"], 4),
                "events_over_filter": round(med["events"] / med["filter"], 4),
                "events_rounds_ms": [round(v, 4) for v in per_round["events"]],
                "statistics_rounds_ms": [round(v, 4) for v in per_round["statistics"]],
                "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
                "prob_crossed_median": round(float(np.median(ev["cdf"][:, -1])), 4),
                "events_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + 3 * d + N_PTS * d) / 1e6, 1),
                "statistics_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + 3 * d) / 1e6, 1)}
    if job in MOMENTS:
        _, n_paths, stride = MOMENTS[job]
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5),
                    "moments": lambda: c.particle_moments(n_paths, 1, stride=stride, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        n_keep = (N_PTS - 1) // stride + 1
        assert all(np.array_equal(res0["filter"][k], res0["moments"][k]) for k in ("log_w", "state", "ess", "resampled"))
        assert res0["moments"]["moments"].shape == (B, n_keep, 2, d) and np.all(np.isfinite(res0["moments"]["moments"]))
        lineage = res0["moments"]["lineage_ess"]
        del res0["moments"]["moments"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        blocks = (n_paths + 63) // 64 if d > 4 else (n_paths + 255) // 256
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "moments", "n_paths": n_paths, "ess_fraction": 0.5,
                "stride": stride, "moments_ms_per_call": round(med["moments"], 4), "filter_ms_per_call": round(med["filter"], 4),
                "ratio": round(med["moments"] / med["filter"], 4),
                "moments_rounds_ms": [round(v, 4) for v in per_round["moments"]],
                "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
                "lineage_ess_first_stretch_median": round(float(np.median(lineage[:, 0])), 2),
                "lineage_ess_last_stretch_median": round(float(np.median(lineage[:, -1])), 2),
                "partial_buffer_mb": round(8.0 * B * blocks * n_keep * 2 * d / 1e6, 1),
                "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_keep * 2 * d) / 1e6, 1)}
    if job in COV:
        _, n_paths, stride = COV[job]
        calls_of = {"covariance": lambda: c.particle_covariance(n_paths, 1, stride=stride, ess_fraction=0.5),
                    "moments": lambda: c.particle_moments(n_paths, 1, stride=stride, ess_fraction=0.5),
                    "filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        n_keep = (N_PTS - 1) // stride + 1
        cov, mom = res0["covariance"], res0["moments"]
        assert all(np.array_equal(res0["filter"][k], cov[k]) for k in ("log_w", "state", "ess", "resampled"))
        assert np.array_equal(cov["lineage_ess"], mom["lineage_ess"])
        assert cov["second"].shape == (B, n_keep, d, d) and cov["mean"].shape == (B, n_keep, d) and np.all(np.isfinite(cov["second"]))
        assert np.array_equal(cov["second"], np.swapaxes(cov["second"], 2, 3))
        big = mom["moments"][:, :, 1]
        assert np.all(np.abs(np.diagonal(cov["second"], axis1=2, axis2=3) - big) <= 1e-9 * big)
        lineage = cov["lineage_ess"]
        del cov, mom, big, res0["covariance"]["second"], res0["moments"]["moments"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        blocks = (n_paths + 63) // 64 if d > 4 else (n_paths + 255) // 256
        packed = d + d * (d + 1) // 2
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "covariance", "n_paths": n_paths, "ess_fraction": 0.5,
                "stride": stride, "covariance_ms_per_call": round(med["covariance"], 4), "moments_ms_per_call": round(med["moments"], 4),
                "filter_ms_per_call": round(med["filter"], 4),
                "ratio_to_moments": round(med["covariance"] / med["moments"], 4), "ratio_to_filter": round(med["covariance"] / med["filter"], 4),
                "covariance_rounds_ms": [round(v, 4) for v in per_round["covariance"]],
                "moments_rounds_ms": [round(v, 4) for v in per_round["moments"]],
                "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
                "lineage_ess_first_stretch_median": round(float(np.median(lineage[:, 0])), 2),
                "lineage_ess_last_stretch_median": round(float(np.median(lineage[:, -1])), 2),
                "partial_buffer_mb": round(8.0 * B * blocks * n_keep * packed / 1e6, 1),
                "moments_partial_buffer_mb": round(8.0 * B * blocks * n_keep * 2 * d / 1e6, 1),
                "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_keep * d * (d + 1)) / 1e6, 1),
                "moments_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_keep * 2 * d) / 1e6, 1)}
    if job in MARG:
        from vgpa_amd.particles import gaussian_ladder
        _, n_paths, stride = MARG[job]
        mt, st = np.asarray(c.fetch("mt")).reshape(B, N_PTS, d), np.asarray(c.fetch("st")).reshape(B, N_PTS, d, d)
        ladders = np.stack([gaussian_ladder(mt[p], st[p], n_levels) for p in range(B)])
        del mt, st
        calls_of = {"moments": lambda: c.particle_moments(n_paths, 1, stride=stride, ess_fraction=0.5),
                    "marginals": lambda: c.particle_marginals(n_paths, 1, ladders, stride=stride, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        n_keep = (N_PTS - 1) // stride + 1
        mg, mom = res0["marginals"], res0["moments"]
        assert all(np.array_equal(mom[k], mg[k]) for k in ("log_w", "state", "ess", "resampled", "lineage_ess"))
        assert mg["mass"].shape == (B, n_keep, d, n_levels + 1) and mg["mass"].dtype == np.uint64
        total = mg["q_final"].sum(axis=1, dtype=np.uint64)
        assert np.all(mg["mass"].sum(axis=3, dtype=np.uint64) == total[:, None, None])
        # the mean of the histogram (bin centres; the end bins at their level) against the moments' mean, in units of the ladder's step
        step = ladders[:, :, 1] - ladders[:, :, 0]
        centres = np.concatenate((ladders[:, :, :1], 0.5 * (ladders[:, :, 1:] + ladders[:, :, :-1]), ladders[:, :, -1:]), axis=2)
        few = slice(0, min(B, 16))      # (on a few problems: at stride 1 the masses of job a are 5 GB)
        hist_mean = np.einsum("pkdb,pdb->pkd", mg["mass"][few].astype(float), centres[few]) / total[few].astype(float)[:, None, None]
        off = float(np.max(np.abs(hist_mean - mom["moments"][few, :, 0]) / step[few, None, :]))
        outside = float(np.max((mg["mass"][few, ..., 0] + mg["mass"][few, ..., -1]).astype(float) / total[few].astype(float)[:, None, None]))
        del mg, mom, hist_mean, centres, res0["marginals"]["mass"], res0["moments"]["moments"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "marginals", "n_paths": n_paths, "ess_fraction": 0.5,
                "stride": stride, "levels": n_levels, "marginals_ms_per_call": round(med["marginals"], 4),
                "moments_ms_per_call": round(med["moments"], 4), "ratio": round(med["marginals"] / med["moments"], 4),
                "marginals_rounds_ms": [round(v, 4) for v in per_round["marginals"]],
                "moments_rounds_ms": [round(v, 4) for v in per_round["moments"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["moments"]["resampled"].mean()), 3),
                "histogram_mean_off_by_steps_max": round(off, 4), "mass_in_the_end_bins_max": round(outside, 6),
                "up_mb": round(8.0 * B * d * n_levels / 1e6, 2),
                "d2h_mb": round(8.0 * B * (n_paths * (2 + d) + n_keep * d * (n_levels + 1)) / 1e6, 1),
                "moments_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_keep * 2 * d) / 1e6, 1)}
    if job in LAG:
        _, n_paths, stride = LAG[job]
        n_keep = (N_PTS - 1) // stride + 1
        anchors = np.arange(LAG_ANCHORS) * (12 * stride)
        rows, every = anchors // stride, np.arange(n_paths)

        def on_the_host():
            res = c.particle_paths(n_paths, 1, n_paths, stride=stride, ess_fraction=0.5, slots=every)
            lw, paths = res["log_w"], res["paths"]
            w = np.exp(lw - lw.max(axis=1, keepdims=True))
            w /= w.sum(axis=1, keepdims=True)
            mean, cross = np.einsum("pi,pikd->pkd", w, paths), np.empty((B, LAG_ANCHORS, n_keep, d, d))
            for p in range(B):
                flat = paths[p].reshape(n_paths, n_keep * d)
                for q, r in enumerate(rows):      # (W x(s))^T X: (D, n) @ (n, n_keep D)
                    cross[p, q] = np.transpose(((w[p][:, None] * paths[p, :, r]).T @ flat).reshape(d, n_keep, d), (1, 2, 0))
            return {"mean": mean, "cross": cross}

        def host_ms(f):
            t0 = time.perf_counter()
            f()
            return 1e3 * (time.perf_counter() - t0)
        dev0, host0 = c.particle_lag_covariance(n_paths, 1, anchors, stride=stride, ess_fraction=0.5), on_the_host()
        scale = np.abs(host0["cross"]).max()
        off = float(np.abs(dev0["cross"] - host0["cross"]).max() / scale)
        assert dev0["cross"].shape == (B, LAG_ANCHORS, n_keep, d, d) and off < 1e-12, off
        del dev0, host0
        per_round = {"lag": [], "lag_host_clock": [], "paths_and_host": []}
        for _ in range(rounds):
            ms = {k: [] for k in per_round}
            for _ in range(calls):
                ms["lag"].append(tm.ms(lambda: c.particle_lag_covariance(n_paths, 1, anchors, stride=stride, ess_fraction=0.5)))
                ms["lag_host_clock"].append(host_ms(lambda: c.particle_lag_covariance(n_paths, 1, anchors, stride=stride, ess_fraction=0.5)))
                ms["paths_and_host"].append(host_ms(on_the_host))
            for k in per_round:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "lag_covariance", "n_paths": n_paths, "ess_fraction": 0.5,
                "stride": stride, "anchors": anchors.tolist(), "lag_ms_per_call": round(med["lag"], 4),
                "lag_host_clock_ms_per_call": round(med["lag_host_clock"], 4), "paths_and_host_ms_per_call": round(med["paths_and_host"], 4),
                "ratio_host_way_to_lag": round(med["paths_and_host"] / med["lag_host_clock"], 3),
                "lag_rounds_ms": [round(v, 4) for v in per_round["lag"]],
                "paths_and_host_rounds_ms": [round(v, 4) for v in per_round["paths_and_host"]],
                "largest_difference_over_largest_entry": off,
                "contraction_gflop": round(2.0 * B * LAG_ANCHORS * n_keep * n_paths * d * d / 1e9, 3),
                "trajectories_on_device_mb": round(8.0 * B * n_paths * n_keep * d / 1e6, 1),
                "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_keep * d * (1 + LAG_ANCHORS * d)) / 1e6, 1),
                "host_way_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_paths * n_keep * d) / 1e6, 1)}
    if job in PATHS:
        _, n_paths, n_draw = PATHS[job]
        stride = paths_stride
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5),
                    "paths": lambda: c.particle_paths(n_paths, 1, n_draw, stride=stride, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        n_keep = (N_PTS - 1) // stride + 1
        assert all(np.array_equal(res0["filter"][k], res0["paths"][k]) for k in ("log_w", "state", "ess", "resampled"))
        assert res0["paths"]["paths"].shape == (B, n_draw, n_keep, d) and np.all(np.isfinite(res0["paths"]["paths"]))
        table = res0["paths"]["slots"]
        if stride == 1:                                   # (the last point of every trajectory is its final slot's particle)
            assert np.array_equal(res0["paths"]["paths"][:, :, -1], np.take_along_axis(res0["paths"]["state"], table[:, -1, :, None].astype(np.int64), axis=1))
        distinct = [float(np.median([np.unique(row).size for row in table[:, j]])) for j in (0, table.shape[1] - 1)]
        del res0["paths"]["paths"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "paths", "n_paths": n_paths, "n_draw": n_draw, "ess_fraction": 0.5,
                "stride": stride, "paths_ms_per_call": round(med["paths"], 4), "filter_ms_per_call": round(med["filter"], 4),
                "ratio": round(med["paths"] / med["filter"], 4),
                "paths_rounds_ms": [round(v, 4) for v in per_round["paths"]],
                "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
                "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
                "distinct_first_stretch_median": distinct[0], "distinct_last_stretch_median": distinct[1],
                "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_draw * n_keep * d) / 1e6, 1)}
    if job in BACKWARD:
        _, n_paths, n_draw = BACKWARD[job]
        stride = paths_stride
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5),
                    "paths": lambda: c.particle_paths(n_paths, 1, n_draw, stride=stride, ess_fraction=0.5),
                    "backward": lambda: c.particle_backward_paths(n_paths, 1, n_draw, stride=stride, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        n_keep = (N_PTS - 1) // stride + 1
        for key in ("log_w", "state", "ess", "resampled"):
            assert np.array_equal(res0["filter"][key], res0["backward"][key]) and np.array_equal(res0["filter"][key], res0["paths"][key]), key
        assert res0["backward"]["paths"].shape == (B, n_draw, n_keep, d) and np.all(np.isfinite(res0["backward"]["paths"]))
        tables = {k: res0[k]["slots"] for k in ("paths", "backward")}
        assert np.array_equal(tables["paths"][:, -1], tables["backward"][:, -1])      # (the same final slots)
        distinct = {k: [float(np.median([np.unique(row).size for row in t[:, j]])) for j in range(t.shape[1])] for k, t in tables.items()}
        del res0["paths"]["paths"], res0["backward"]["paths"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        out = {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "backward", "n_paths": n_paths, "n_draw": n_draw, "ess_fraction": 0.5,
               "stride": stride, "backward_ms_per_call": round(med["backward"], 4), "paths_ms_per_call": round(med["paths"], 4),
               "filter_ms_per_call": round(med["filter"], 4), "ratio_to_paths": round(med["backward"] / med["paths"], 4),
               "ratio_to_filter": round(med["backward"] / med["filter"], 4),
               "backward_rounds_ms": [round(v, 4) for v in per_round["backward"]], "paths_rounds_ms": [round(v, 4) for v in per_round["paths"]],
               "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
               "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
               "distinct_per_stretch_median_backward": distinct["backward"], "distinct_per_stretch_median_genealogy": distinct["paths"],
               "histories_on_device_mb": round(8.0 * B * int(c.n_obs) * n_paths * (d + 1) / 1e6, 1),
               "d2h_mb": round(8.0 * B * (n_paths * (1 + d) + n_draw * n_keep * d) / 1e6, 1)}
        twin_job = job.replace("b", "p", 1) if job[0] == "a" else "bp" + job[2:]
        row = (parent or {}).get((twin_job, stride))
        if row:
            out.update(parent_tree=row["tree"], parent_paths_ms_per_call=row["paths_ms_per_call"], parent_paths_rounds_ms=row["paths_rounds_ms"],
                       parent_filter_ms_per_call=row["filter_ms_per_call"], ratio_to_parent_paths=round(med["backward"] / row["paths_ms_per_call"], 4))
        return out
    if job in SMOOTH:
        _, n_paths = SMOOTH[job]
        stride = N_PTS + 3      # (one kept grid index: the K = n trajectories of the draw's call leave as B n D doubles, not B n n_keep D)
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5),
                    "moments": lambda: c.particle_moments(n_paths, 1, stride=stride, ess_fraction=0.5),
                    "backward_moments": lambda: c.particle_backward_moments(n_paths, 1, stride=stride, ess_fraction=0.5, weights=False),
                    "backward_paths": lambda: c.particle_backward_paths(n_paths, 1, n_paths, stride=stride, ess_fraction=0.5)}
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        for key in ("log_w", "state", "ess", "resampled"):
            assert all(np.array_equal(res0["filter"][key], res0[k][key]) for k in calls_of), key
        got, old = res0["backward_moments"], res0["moments"]
        assert got["moments"].shape == old["moments"].shape and np.all(np.isfinite(got["moments"]))
        ess = {"backward": np.median(got["smoothing_ess"], axis=0), "genealogy": np.median(old["lineage_ess"], axis=0)}
        del res0["backward_paths"]["paths"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        out = {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "backward_moments", "n_paths": n_paths, "ess_fraction": 0.5, "stride": stride,
               "observations": int(c.n_obs), "resampled_share": round(float(res0["filter"]["resampled"].mean()), 3)}
        for k in calls_of:
            out[k + "_ms_per_call"] = round(med[k], 4)
            out[k + "_rounds_ms"] = [round(v, 4) for v in per_round[k]]
        out.update(ratio_to_moments=round(med["backward_moments"] / med["moments"], 4),
                   ratio_to_backward_paths=round(med["backward_moments"] / med["backward_paths"], 4),
                   pass_ms_over_moments=round(med["backward_moments"] - med["moments"], 4),
                   draw_ms_over_filter=round(med["backward_paths"] - med["filter"], 4),
                   smoothing_ess_first_middle=[round(float(ess["backward"][0]), 2), round(float(ess["backward"][ess["backward"].size // 2]), 2)],
                   lineage_ess_first_middle=[round(float(ess["genealogy"][0]), 2), round(float(ess["genealogy"][ess["genealogy"].size // 2]), 2)],
                   histories_on_device_mb=round(8.0 * B * int(c.n_obs) * n_paths * (d + 1) / 1e6, 1))
        return out
    if job in GIBBS:
        _, n_paths = GIBBS[job]
        ref = np.ascontiguousarray(c.particle_paths(n_paths, 2, 1, ess_fraction=0.5)["paths"][:, 0])
        calls_of = {"filter": lambda: c.particle_filter(n_paths, 1, ess_fraction=0.5),
                    "paths": lambda: c.particle_paths(n_paths, 1, 1, ess_fraction=0.5),
                    "conditional": lambda: c.particle_conditional(ref, n_paths, 1, ess_fraction=0.5)}
        if not hasattr(c, "particle_conditional"):      # (this tool copied into a checkout without the entry point: the two calls it has)
            del calls_of["conditional"]
        res0 = {k: f() for k, f in calls_of.items()}      # warm-up (first-use allocations)
        moved = other = None
        flags = res0["filter"]["resampled"].astype(bool)
        if "conditional" in calls_of:
            got = res0["conditional"]
            traj, table = got["trajectory"], got["slots"]
            assert traj.shape == (B, N_PTS, d) and np.all(np.isfinite(traj))
            assert np.array_equal(traj[:, -1], np.take_along_axis(got["state"], table[:, -1, None, None].astype(np.int64), axis=1)[:, 0])
            moved = float(np.mean(np.any(traj != ref, axis=2)))
            flags = got["resampled"].astype(bool)
            # the ancestors of the pinned slot: one more call with the histories, where they are small (at 1024 particles the clouds alone
            # are 8 to 13 GB of host memory: too much for one statistic)
            if 8.0 * B * int(c.n_obs) * n_paths * (d + 1) <= 2.0 ** 30:
                anc = c.particle_conditional(ref, n_paths, 1, ess_fraction=0.5, history=True)["ancestors"]
                other = float(np.mean(anc[:, :, 0][flags] != 0)) if flags.any() else 0.0
                del anc
            del got, traj
        del res0["paths"]["paths"]
        per_round = {k: [] for k in calls_of}
        for _ in range(rounds):
            ms = {k: [] for k in calls_of}
            for _ in range(calls):
                for k, f in calls_of.items():
                    ms[k].append(tm.ms(f))
            for k in calls_of:
                per_round[k].append(float(np.median(ms[k])))
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        out = {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "gibbs", "n_paths": n_paths, "ess_fraction": 0.5, "stride": 1,
               "paths_ms_per_call": round(med["paths"], 4), "filter_ms_per_call": round(med["filter"], 4),
               "paths_rounds_ms": [round(v, 4) for v in per_round["paths"]], "filter_rounds_ms": [round(v, 4) for v in per_round["filter"]],
               "observations": int(c.n_obs), "resampled_share": round(float(flags.mean()), 3),
               "filter_resampled_share": round(float(res0["filter"]["resampled"].mean()), 3),
               "filter_d2h_mb": round(8.0 * B * n_paths * (1 + d) / 1e6, 1), "paths_d2h_mb": round(8.0 * B * (n_paths * (1 + d) + N_PTS * d) / 1e6, 1)}
        if "conditional" in calls_of:
            out.update(conditional_ms_per_call=round(med["conditional"], 4), conditional_rounds_ms=[round(v, 4) for v in per_round["conditional"]],
                       ratio_to_paths=round(med["conditional"] / med["paths"], 4), ratio_to_filter=round(med["conditional"] / med["filter"], 4),
                       share_of_grid_renewed=round(moved, 4), pinned_ancestor_other_slot_share=None if other is None else round(other, 4),
                       up_mb=round(8.0 * B * N_PTS * d / 1e6, 1), d2h_mb=round(8.0 * B * (n_paths * (1 + d) + N_PTS * d) / 1e6, 1))
        row = (parent or {}).get((job, 1))
        if row:
            out.update(parent_tree=row["tree"], parent_filter_ms_per_call=row["filter_ms_per_call"], parent_paths_ms_per_call=row["paths_ms_per_call"],
                       parent_filter_rounds_ms=row["filter_rounds_ms"], parent_paths_rounds_ms=row["paths_rounds_ms"])
            if "conditional" in calls_of:
                out.update(ratio_to_parent_filter=round(med["conditional"] / row["filter_ms_per_call"], 4),
                           ratio_to_parent_paths=round(med["conditional"] / row["paths_ms_per_call"], 4))
        return out
    if job in FILTER:
        _, n_paths, frac = FILTER[job]
        call = lambda: c.particle_filter(n_paths, 1, ess_fraction=frac)      # noqa: E731
        res0 = call()                                 # warm-up (first-use allocations)
        assert res0["log_w"].shape == (B, n_paths) and np.all(np.isfinite(res0["log_w"])) and np.all(np.isfinite(res0["state"]))
        resampled = float(res0["resampled"].mean())
        per_round = [float(np.median([tm.ms(call) for _ in range(calls)])) for _ in range(rounds)]
        return {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": "filter", "n_paths": n_paths, "ess_fraction": frac,
                "ms_per_call": round(float(np.median(per_round)), 4), "rounds_ms": [round(v, 4) for v in per_round],
                "observations": int(c.n_obs), "resampled_share": round(resampled, 3),
                "d2h_mb": round(8.0 * B * n_paths * (1 + d) / 1e6, 1)}
    if weighted:
        call = lambda: c.sample_paths_weighted(n_paths, 1, stride=stride, paths=stored)      # noqa: E731
        out, logw, start = call()                     # warm-up (first-use allocations)
        assert logw.shape == (B, n_paths, 2) and start.shape == (B, n_paths, d) and np.all(np.isfinite(logw)) and np.all(np.isfinite(start))
        assert (out is None) if not stored else (out.shape == (B, n_paths, n_keep, d) and bool(np.all(np.isfinite(out))))
        del out, logw, start
    else:
        call = lambda: c.sample_paths(kind, n_paths, 1, stride=stride)      # noqa: E731
        out = call()                                  # warm-up (first-use allocations)
        assert out.shape == (B, n_paths, n_keep, d) and np.all(np.isfinite(out))
        del out
    per_round = [float(np.median([tm.ms(call) for _ in range(calls)])) for _ in range(rounds)]
    out_bytes = 8.0 * B * n_paths * ((n_keep * d if stored else 0) + ((2 + d) if weighted else 0))
    readers = B * ((n_paths + 63) // 64 if d > 4 else n_paths)
    x_bytes = 8.0 * readers * len_x if kind == "posterior" else 0.0
    res = {"job": job, "model": name, "D": d, "Np": N_PTS, "B": B, "kind": kind, "n_paths": n_paths, "stride": stride,
           "ms_per_call": round(float(np.median(per_round)), 4), "rounds_ms": [round(v, 4) for v in per_round]}
    if weighted:                                      # (no host-loop time: the twin's row has the paths' one)
        res.update(weighted=True, paths_stored=stored)
    else:
        res.update(numpy_ms=round(numpy_ms(p0, x_row, d, kind, n_paths, stride, numpy_problems, B), 1), numpy_problems=numpy_problems)
    res.update({"floor_ms": round((x_bytes + out_bytes) / HBM_BYTES_PER_S * 1e3, 4), "x_gb": round(x_bytes / 1e9, 3),
                "d2h_mb": round(out_bytes / 1e6, 1)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--jobs", default="a,b,c")
    ap.add_argument("--numpy-problems", type=int, default=2)
    ap.add_argument("--filter-problems", type=int, default=0, help="cap on B of the b context's filter jobs (0: none)")
    ap.add_argument("--statistics", action="store_true", help="run the as* and bs* jobs (particle_statistics beside particle_filter)")
    ap.add_argument("--events", action="store_true", help="run the ae* and be* jobs (particle_events beside particle_statistics and particle_filter)")
    ap.add_argument("--moments", action="store_true", help="run the am* and bm* jobs (particle_moments beside particle_filter)")
    ap.add_argument("--covariance", action="store_true", help="run the ac* and bc* jobs (particle_covariance beside particle_moments and particle_filter)")
    ap.add_argument("--marginals", action="store_true", help="run the ah* and bh* jobs (particle_marginals beside particle_moments)")
    ap.add_argument("--levels", type=int, default=31, help="levels per component of the ah* and bh* jobs")
    ap.add_argument("--lag-covariance", action="store_true", help="run the al* and bl* jobs (particle_lag_covariance beside particle_paths and the host's contraction)")
    ap.add_argument("--lag-problems", type=int, default=0, help="cap on B of the a context's lag-covariance job (0: none)")
    ap.add_argument("--paths", action="store_true", help="run the ap* and bp* jobs (particle_paths beside particle_filter)")
    ap.add_argument("--paths-strides", default="1,10", help="strides of the ap* and bp* jobs: each job runs once per stride")
    ap.add_argument("--backward", action="store_true", help="run the ab* and bb* jobs (particle_backward_paths beside particle_paths and particle_filter)")
    ap.add_argument("--backward-moments", action="store_true", help="run the aw*, bw* and ow* jobs (particle_backward_moments beside particle_moments, particle_backward_paths with K = n and particle_filter)")
    ap.add_argument("--smooth-problems", type=int, default=8, help="B of the aw*, bw* and ow* jobs")
    ap.add_argument("--gibbs", action="store_true", help="run the ag* and bg* jobs (particle_conditional beside particle_paths and particle_filter)")
    ap.add_argument("--parent-json", default="", help="output of the parent commit's --paths run of the same jobs: its times are reported beside")
    ap.add_argument("--forecast", action="store_true", help="run the forecast job (particle_forecast from a given cloud beside the model-kind sampler)")
    ap.add_argument("--forecast-problems", type=int, default=512)
    ap.add_argument("--forecast-particles", type=int, default=4096)
    ap.add_argument("--forecast-horizon", type=int, default=1000)
    args = ap.parse_args()
    if args.forecast:
        out = {"tool": "bench_sample_paths", "tree": tree(), "unit": "ms per call (device events around the call)",
               "jobs": [run_forecast(args.forecast_problems, args.forecast_particles, args.forecast_horizon, args.rounds, args.calls)]}
        print(json.dumps(out), flush=True)
        return
    if args.statistics:
        args.jobs = ",".join(sorted(STATS))
    if args.events:
        args.jobs = ",".join(sorted(EVENTS))
    if args.moments:
        args.jobs = ",".join(sorted(MOMENTS))
    if args.covariance:
        args.jobs = ",".join(sorted(COV))
    if args.marginals and args.jobs == "a,b,c":
        args.jobs = ",".join(sorted(MARG))
    if args.lag_covariance and args.jobs == "a,b,c":
        args.jobs = ",".join(sorted(LAG))
    if args.paths:
        args.jobs = ",".join(sorted(PATHS))
    if args.backward and args.jobs == "a,b,c":
        args.jobs = ",".join(sorted(BACKWARD))
    if args.backward_moments and args.jobs == "a,b,c":
        args.jobs = ",".join(sorted(SMOOTH))
    if args.gibbs and args.jobs == "a,b,c":
        args.jobs = ",".join(sorted(GIBBS))
    parent = {}
    if args.parent_json:      # (one JSON line per run of the parent's tool; a later run of a job replaces an earlier one)
        with open(args.parent_json) as fh:
            for line in fh:
                if line.strip().startswith("{"):
                    doc = json.loads(line)
                    for row in doc.get("jobs", []):
                        parent[(row["job"], row.get("stride", 1))] = dict(row, tree=doc.get("tree", "unknown"))
    strides = [int(v) for v in args.paths_strides.split(",") if v]
    cache = {}
    out = {"tool": "bench_sample_paths", "tree": tree(), "unit": "ms per call (device events around the call)", "jobs": []}
    for job in [j for j in args.jobs.split(",") if j]:
        for stride in (strides if job in PATHS or job in BACKWARD else [1]):
            out["jobs"].append(run(job, args.rounds, args.calls, args.numpy_problems, cache, args.filter_problems, stride, parent, args.levels, args.lag_problems, args.smooth_problems))
    for c, _, _, _, tm in cache.values():
        tm.close()
        c.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
