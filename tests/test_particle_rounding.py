"""
GPU suite (-m gpu): the particle half -- the walks of vgpa_amd/csrc/sample.hip, k_forecast_l96 and the k_pf_* reductions -- held to ROUNDING
ERROR, step by step.  Everything but the device calls comes from test_particle_rounding_cpu.py: the case tables, the inputs, the floors,
the longdouble restatements (tests/extended_ref.py) and the conditions on the cases, asserted there without a device.

The principle: every comparison starts from data the device itself returned, or data the host supplied, and spans at most one step of the
recursion or one reduction, so that no path's chaos enters; every compared quantity q then meets the project's bound

    err_k(q) <= FACTOR * max(err_o(q), floor(q))                                               FACTOR = 32

err_k the kernel, err_o the fp64 numpy restatement of the same step or reduction on the same inputs, both against the longdouble
restatement, the differences taken in longdouble; the floors as listed in test_particle_rounding_cpu.py.  Every comparison prints err_o,
err_k (in units of the floor) and their ratio err_k / max(err_o, floor); test_print_worst prints the worst ratio per kernel family and
quantity at the end.

  A  the normals: the start of sample_paths_weighted on a context with m0 = 0, S0 = I is the device's xi of counter (0, path, p, j) bit for bit
     (adding zeros and multiplying by one are exact); k_sample_small, k_sample_mfma<16 | 32 | 48 | 64>, 65 536 paths, k_pf_start
  B  one step of every walk: every consecutive pair of every stride-1 path -- posterior kind (diagonal and dense factor, benign and stiff),
     model kind, the lineage walk under resampling, the backward-simulation walk with its reloaded states, the forecast from a host-given
     cloud (members, state_end)
  C  the path term and the observation term of sample_paths_weighted from its own stored paths; particle_filter(ess_fraction=0)'s log_w
  D  the rows of particle_statistics from the stored paths (no resampling) and from particle_paths' lineages (resampling)
  E  reductions of returned data: the mean of the rows, the forecast's moments at every kept step, particle_moments / particle_covariance and
     their lineage_ess from the lineages, the final log-weights and the slot table
Measured on an MI355X (profiles/particle_rounding_gputests.log; 187 cases, 12 s): no kernel exceeded its bound, and the fp64 restatement stays
within the floors there too (worst err_o 0.97), so every bound was 32 floors.  Worst ratio per quantity:
  xi 0.47; step 0.76 (k_sample_small<Lineage | Backward>; k_sample_mfma 0.73, k_sample_l96 0.65, k_forecast_l96 0.58); path term 0.38; obs term
  0.44, under a dense R of cond 1e4 0.07; filter log_w 0.29; rows Q 0.52, G 0.24, H 1.05; their mean 0.85; forecast moments 0.97; replay sums:
  sum W x 0.26, sum W x^2 0.27, sum W x x^T 0.34, lineage_ess 0.24
Not here: the ess histories and the log-weights across a resampling (no device output isolates their inputs); the Gumbel-max draw of
k_pf_backward and the resampling indices (compared exactly, under gap conditions, by the older tests).
"""
import numpy as np
import pytest

import vgpa_amd as va
from test_gpu_edge_cases import gpu_context, make_problem
from test_particle_filter_cpu import SEED as PF_SEED, case
from test_particle_rounding_cpu import (B, BACKWARD_RUNS, BIG_NORMALS, BIG_PATHS, CENTRE, DT, FORECAST_CASES, FORECAST_INDEX0, MODEL_WALKS, MOMENT_SHAPES, MOMENT_SIZES,
                                        MOMENT_WEIGHTS, N_PATHS, NORMAL_DIMS, OBS_VARIANTS, POSTERIOR_WALKS, RESAMPLED_RUNS, SEED, SEED_W,
                                        SMOOTHING_RUNS, SMOOTHING_STRIDES, SMOOTHING_TAGS, START_DIMS, STATS_TAGS, WEIGHT_SIZES, Walk, _model_of, _split, _sigma_diag,
                                        backward_case, check_backward, check_forecast, check_log_weights, check_moments, check_normals, check_rows, check_smoothing, check_steps,
                                        check_walk, check_weighted_sum, check_weights, forecast_inputs, lineage_words, moment_case, obs_variant,
                                        smoothing_case, walk_id, walk_inputs, xr)
from test_path_weights_cpu import TAGS

pytestmark = pytest.mark.gpu
WORST = {}                 # (kernel family, quantity) -> the worst ratio err_k / max(err_o, floor) of this process's run


def _family(d, walk=""):
    return ("k_sample_small" if d <= 4 else "k_sample_mfma") + (f"<{walk}>" if walk else "")


def walk_context(c, identity_start=False, obs_at=1, batch=B):
    """the context of a walk case: `batch` problems with their own theta and Sigma (walk_inputs)"""
    inp, d = walk_inputs(c), c.d
    kw = {}
    if c.model != "NONE":
        kw = dict(theta=inp.theta[0], obs_t=np.array([obs_at], dtype=np.int64), obs_y=inp.obs_y, obs_noise=inp.obs_noise)
    ctx = va.Context(c.model, "euler", d, c.n_pts, DT, sigma=inp.sigma[0], m0=np.zeros(d) if identity_start else inp.m0,
                     s0=np.eye(d) if identity_start else inp.s0, batch=batch, **kw)
    if c.model != "NONE":      # (no stochastic model: no per-problem parameters; walk_inputs gives its problems one Sigma)
        ctx.set_problem_params(theta=inp.theta[:batch], sigma=inp.sigma[:batch])
    return ctx


@pytest.fixture(scope="module")
def contexts():
    """one bare context per tag of test_particle_filter_cpu.case / smoothing_case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _ctx(cache, tag):
    if tag not in cache:
        q = smoothing_case(tag)[0]
        d = int(q.dim_d)
        cache[tag] = va.Context(q.model, getattr(q, "method", "euler"), d, int(q.n_pts), float(q.dt), sigma=np.reshape(np.asarray(q.sigma, dtype=float), (d, d)),
                                theta=np.atleast_1d(q.theta), m0=np.atleast_1d(q.m0), s0=np.reshape(np.asarray(q.s0, dtype=float), (d, d)),
                                obs_t=q.obs_t, obs_y=q.obs_y, obs_noise=np.reshape(np.asarray(q.obs_noise, dtype=float), (d, d)),
                                obs_h=None if getattr(q, "obs_h", None) is None else np.reshape(np.asarray(q.obs_h, dtype=float), (d, d)))
    return cache[tag]


# ---- A: the normals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", NORMAL_DIMS)
def test_normals(d):
    c = Walk("posterior", _model_of(d), d, 5, "benign", "diag")
    ctx = walk_context(c, identity_start=True)
    paths, _, start = ctx.sample_paths_weighted(N_PATHS, SEED, x=walk_inputs(c).x)
    ctx.close()
    assert start.shape == (B, N_PATHS, d) and np.array_equal(start, paths[:, :, 0])
    fails = []
    for p in range(B):
        fails += check_normals(WORST, f"D={d} p={p}", _family(d, "start"), start[p], SEED, 0, np.arange(N_PATHS), p, d)
    assert not fails, fails


def test_normals_at_the_extremes():
    """65 536 paths at D = 4, Np = 2: u1 near 0 and 1, u2 near every multiple of 1/4 (asserted on the host's Philox by the CPU module)"""
    c = BIG_NORMALS
    ctx = walk_context(c, identity_start=True, batch=1)
    paths, _, start = ctx.sample_paths_weighted(BIG_PATHS, SEED, x=walk_inputs(c).x[:1])
    ctx.close()
    assert np.array_equal(start, paths[:, :, 0])
    fails = check_normals(WORST, "65536 paths", _family(c.d, "start"), start[0], SEED, 0, np.arange(BIG_PATHS), 0, c.d)
    assert not fails, fails


@pytest.mark.parametrize("d", START_DIMS)
def test_normals_of_the_filters_start(d):
    """an observation at grid index 0: clouds[0] is what k_pf_start drew"""
    c = Walk("posterior", _model_of(d), d, 5, "benign", "diag")
    ctx = walk_context(c, identity_start=True, obs_at=0)
    got = ctx.particle_filter(N_PATHS, SEED, ess_fraction=0.0, x=walk_inputs(c).x, history=True)
    ctx.close()
    fails = []
    for p in range(B):
        fails += check_normals(WORST, f"D={d} p={p}", "k_pf_start", got["clouds"][p, 0], SEED, 0, np.arange(N_PATHS), p, d)
    assert not fails, fails


# ---- B: one step of every walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", POSTERIOR_WALKS, ids=walk_id)
def test_posterior_steps(c):
    ctx = walk_context(c)
    paths = ctx.sample_paths("posterior", N_PATHS, SEED, x=walk_inputs(c).x)
    ctx.close()
    assert paths.shape == (B, N_PATHS, c.n_pts, c.d)
    fails = []
    for p in range(B):
        fails += check_walk(WORST, f"{walk_id(c)} p={p}", _family(c.d, "Plain" + (", dense R" if c.sigma == "dense" else "")), c, p, paths[p])
    assert not fails, fails


@pytest.mark.parametrize("c", MODEL_WALKS, ids=walk_id)
def test_model_steps(c):
    ctx = walk_context(c)
    paths = ctx.sample_paths("model", N_PATHS, SEED)
    ctx.close()
    family = "k_sample_small<Plain>, model" if c.d <= 4 else "k_sample_l96" + (", dense R" if c.sigma == "dense" else "")
    fails = []
    for p in range(B):
        fails += check_walk(WORST, f"{walk_id(c)} p={p}", family, c, p, paths[p])
    assert not fails, fails


@pytest.mark.parametrize("c", FORECAST_CASES, ids=walk_id)
def test_forecast_steps(c):
    """from a host-given cloud, no filter: the members of all slots at stride 1, state_end, and the moments of every kept step as a reduction
    of the members the device returned"""
    inp, d = forecast_inputs(c), c.d
    ctx = va.Context(c.model, "euler", d, 41, DT, sigma=inp.sigma[0], theta=inp.theta[0], m0=np.full(d, CENTRE[c.model]), s0=0.2 * np.eye(d),
                     obs_t=np.array([2], dtype=np.int64), obs_y=np.full((1, d), CENTRE[c.model]), obs_noise=np.eye(d), batch=B)
    ctx.set_problem_params(theta=inp.theta, sigma=inp.sigma)
    out = ctx.particle_forecast(c.horizon, seed=SEED, stride=1, cloud=inp.cloud, log_w=inp.log_w, index0=FORECAST_INDEX0, slots=np.arange(c.n))
    ctx.close()
    assert out["members"].shape == (B, c.n, c.horizon + 1, d) and out["state_end"].shape == (B, c.n, d)
    family = "k_sample_small<Forecast>" if d <= 4 else "k_forecast_l96"
    fails = []
    for p in range(B):
        local = {}
        fails += check_forecast(local, f"{walk_id(c)} p={p}", c, p, out["members"][p], out["state_end"][p])
        WORST[(family, "step")] = max(WORST.get((family, "step"), 0.0), local[("forecast", "step")])
        for h in range(c.horizon + 1):
            local = {}
            fails += check_moments(local, f"{walk_id(c)} p={p} h={h}", out["members"][p][:, h], inp.log_w[p], out["moments"][p, h])
            for (_, quantity), r in local.items():
                WORST[(family, quantity)] = max(WORST.get((family, quantity), 0.0), r)
    assert not fails, fails


# ---- C: log-weights from the device's own paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("n", WEIGHT_SIZES)
@pytest.mark.parametrize("tag", TAGS)
def test_weights_from_the_stored_paths(contexts, tag, n, start):
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    paths, logw, first = ctx.sample_paths_weighted(n, SEED_W, x=x, x0=s0)
    assert np.array_equal(first, paths[:, :, 0]) and np.all(np.isfinite(logw))
    d = int(q.dim_d)
    fails = check_weights(WORST, f"{tag} n={n} {start}", _family(d, "Weighted"), q, x, paths[0], logw[0, :, 0], logw[0, :, 1])
    # no prior: the initial term is 0 for either start, and log_w = -c + path + obs, summed segment by segment
    got = ctx.particle_filter(n, SEED_W, ess_fraction=0.0, x=x, x0=s0)
    assert np.array_equal(got["state"][0], paths[0][:, -1]) and not got["resampled"].any()
    fails += check_log_weights(WORST, f"{tag} n={n} {start}", q, x, paths[0], got["log_w"][0])
    assert not fails, fails


@pytest.mark.parametrize("model,d", OBS_VARIANTS)
def test_weights_under_a_dense_observation_model(model, d):
    """dense R of condition 1e4, H = I + 0.1 noise, observations at the grid indices 0 and Np - 1 and at adjacent indices"""
    q, x = obs_variant(model, d)
    ctx = gpu_context(q)
    fails = []
    for n in WEIGHT_SIZES:
        paths, logw, first = ctx.sample_paths_weighted(n, SEED_W, x=x)
        assert np.array_equal(first, paths[:, :, 0])
        fails += check_weights(WORST, f"{model}{d} n={n}", _family(d, "Weighted") + ", dense R, H", q, x, paths[0], logw[0, :, 0], logw[0, :, 1])
    ctx.close()
    assert not fails, fails


# ---- D: the statistics rows; E: their mean -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", STATS_TAGS)
def test_statistics_rows_without_resampling(contexts, tag):
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    paths, _, _ = ctx.sample_paths_weighted(N_PATHS, PF_SEED, x=x, x0=x0)
    got = ctx.particle_statistics(N_PATHS, PF_SEED, ess_fraction=0.0, x=x, x0=x0, per_particle=True)
    assert np.array_equal(got["state"][0], paths[0][:, -1]) and not got["resampled"].any()
    d = int(q.dim_d)
    fails = check_rows(WORST, tag, _family(d, "SegmentStats"), q, paths[0], got["stats"][0])
    fails += check_weighted_sum(WORST, tag, "k_pf_stats_mean", "mean of rows", got["log_w"][0], got["stats"][0], got["mean"][0])
    assert not fails, fails


def _lineages(ctx, q, x, x0, n, frac):
    """particle_paths(slots=arange(n), stride=1) with the bit-equalities that license its lineages: paths[t_j] == clouds[j][s_j],
    paths[Np - 1] == state[s_c], the filter's four results equal across the entry points"""
    lin = ctx.particle_paths(n, PF_SEED, n, stride=1, ess_fraction=frac, x=x, x0=x0, slots=np.arange(n))
    flt = ctx.particle_filter(n, PF_SEED, ess_fraction=frac, x=x, x0=x0, history=True)
    for key in ("log_w", "state", "ess", "resampled"):
        assert np.array_equal(lin[key], flt[key]), key
    paths, table = lin["paths"][0], lin["slots"][0]
    obs_t = np.asarray(q.obs_t, dtype=np.int64).ravel()
    assert table.shape == (obs_t.size + 1, n) and np.array_equal(table[-1], np.arange(n))
    assert np.array_equal(paths[:, -1], flt["state"][0][table[-1]])
    for j, t in enumerate(obs_t):
        assert np.array_equal(paths[:, t], flt["clouds"][0, j][table[j]]), j
    return lin, flt


@pytest.mark.parametrize("run", RESAMPLED_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_lineage_walk_and_rows_with_resampling(contexts, run):
    """the lineage walk's every step (B), the rows of the slots' lineages (D) and their mean (E)"""
    tag, start, n, frac = run
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    lin, flt = _lineages(ctx, q, x, x0, n, frac)
    paths, table = lin["paths"][0], lin["slots"][0]
    assert flt["resampled"].any() and len(set(table[0].tolist())) >= 2
    d, n_pts = int(q.dim_d), int(q.n_pts)
    lin_a, off_b = _split(q, x)
    drift = lambda v, T: xr.posterior_drift(lin_a.reshape(-1, d, d)[:-1], off_b.reshape(-1, d)[:-1], v, T)      # noqa: E731
    fac = np.linalg.cholesky(_sigma_diag(q) * float(q.dt))
    fails = check_steps(WORST, tag, _family(d, "Lineage"), paths[:, :-1], paths[:, 1:], np.arange(1, n_pts), lineage_words(q.obs_t, table, n_pts), 0,
                        PF_SEED, fac, drift)
    got = ctx.particle_statistics(n, PF_SEED, ess_fraction=frac, x=x, x0=x0, per_particle=True)
    for key in ("log_w", "state", "ess", "resampled"):
        assert np.array_equal(got[key], flt[key]), key
    fails += check_rows(WORST, tag, _family(d, "SegmentStats") + ", resampled", q, paths, got["stats"][0])
    fails += check_weighted_sum(WORST, tag, "k_pf_stats_mean", "mean of rows", got["log_w"][0], got["stats"][0], got["mean"][0])
    assert not fails, fails


@pytest.mark.parametrize("run", BACKWARD_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_backward_walk_steps(contexts, run):
    """particle_backward_paths: a step behind a resampled observation starts from the reloaded particle clouds_j[anc_j[s_{j+1}]] out of the
    filter's history, every other one from the stored point; the table is the device's own"""
    tag, start, n, frac = run
    q, x, x0 = backward_case(tag)
    ctx = gpu_context(q) if tag.startswith("tight") else _ctx(contexts, tag)
    flt = ctx.particle_filter(n, PF_SEED, ess_fraction=frac, x=x, x0=x0, history=True)
    bw = ctx.particle_backward_paths(n, PF_SEED, n, stride=1, ess_fraction=frac, x=x, x0=x0, slots=np.arange(n))
    if tag.startswith("tight"):
        ctx.close()
    for key in ("log_w", "state", "ess", "resampled"):
        assert np.array_equal(bw[key], flt[key]), key
    assert flt["resampled"].any() and np.array_equal(bw["slots"][0][-1], np.arange(n))
    fails = check_backward(WORST, tag, _family(int(q.dim_d), "Backward"), q, x, bw["paths"][0], bw["slots"][0], flt["ancestors"][0], flt["clouds"][0], PF_SEED)
    assert not fails, fails


# ---- E: reductions of returned data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", MOMENT_SHAPES)
def test_forecast_moments_at_horizon_zero(model, d):
    """k_pf_normalise and the sums of the cloud launch, from a host-given cloud and log-weights; the cloud comes back unchanged"""
    q = make_problem(model, d, 41, method="euler")[0]
    ctx = gpu_context(q)
    family = ("k_sample_small<Forecast>" if d <= 4 else "k_forecast_l96") + ", H = 0"
    fails = []
    for n in MOMENT_SIZES:
        for weights in MOMENT_WEIGHTS:
            cloud, lw = moment_case(model, d, n, weights)
            out = ctx.particle_forecast(0, seed=SEED, cloud=cloud, log_w=lw, index0=FORECAST_INDEX0)
            assert out["moments"].shape == (1, 1, 2, d) and np.array_equal(out["state_end"][0], cloud)
            local = {}
            fails += check_moments(local, f"{model}{d} n={n} {weights}", cloud, lw, out["moments"][0, 0])
            for (_, quantity), r in local.items():
                WORST[(family, quantity)] = max(WORST.get((family, quantity), 0.0), r)
    ctx.close()
    assert not fails, fails


def _smoothing(ctx, q, x, x0, n, frac, label, family_tail):
    lin, flt = _lineages(ctx, q, x, x0, n, frac)
    paths, table, d = lin["paths"][0], lin["slots"][0], int(q.dim_d)
    fails = []
    for stride in SMOOTHING_STRIDES:
        mom = ctx.particle_moments(n, PF_SEED, stride=stride, ess_fraction=frac, x=x, x0=x0)
        cov = ctx.particle_covariance(n, PF_SEED, stride=stride, ess_fraction=frac, x=x, x0=x0)
        for key in ("log_w", "state", "ess", "resampled"):
            assert np.array_equal(mom[key], flt[key]) and np.array_equal(cov[key], flt[key]), key
        assert np.array_equal(mom["lineage_ess"], cov["lineage_ess"])
        assert np.array_equal(cov["second"], np.swapaxes(cov["second"], -1, -2))
        fails += check_smoothing(WORST, f"{label} stride {stride}", _family(d, "Replay") + family_tail, flt["log_w"][0], table, paths, stride,
                                 mom["moments"][0][:, 0], mom["moments"][0][:, 1], mom["lineage_ess"][0])
        fails += check_smoothing(WORST, f"{label} stride {stride}", _family(d, "ReplayCov") + family_tail, flt["log_w"][0], table, paths, stride,
                                 cov["mean"][0], cov["second"][0], cov["lineage_ess"][0])
    return fails, flt, table


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("tag", SMOOTHING_TAGS)
def test_smoothing_sums_without_resampling(contexts, tag, n):
    q, x, x0 = smoothing_case(tag)
    fails, flt, _ = _smoothing(_ctx(contexts, tag), q, x, x0, n, 0.0, f"{tag} n={n}", "")
    assert not flt["resampled"].any()
    assert not fails, fails


@pytest.mark.parametrize("run", SMOOTHING_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_smoothing_sums_with_resampling(contexts, run):
    tag, start, n, frac = run
    q, x, x0 = case(tag)
    fails, flt, table = _smoothing(_ctx(contexts, tag), q, x, x0, n, frac, tag, ", resampled")
    assert flt["resampled"].any() and len(set(table[0].tolist())) >= 2
    assert not fails, fails


def test_print_worst():
    """(last: the table of this run)"""
    print("WORST ratio err_k / max(err_o, floor) per kernel family and quantity:")
    for (family, quantity), r in sorted(WORST.items()):
        print(f"WORST  {family:45s} {quantity:14s} {r:8.2f}")
