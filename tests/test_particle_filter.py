"""
The guided particle filter on the GPU (vgpa_particle_filter).

Reference: test_particle_filter_cpu.particle_filter_numpy, evaluated with each problem's own rows and computed once per case (its cache is
shared with the CPU tests and never written).  `resampled` and `ancestors` are compared exactly -- test_particle_filter_cpu's margin
condition holds for every (case, n, seed) used here -- and ess, the log-weights, the final particles and the clouds to 1e-9: relative for
ess, |got - want| <= 1e-9 (1 + scale) for the log-weights (scale as in test_path_weights.py, carried through resamplings by the
restatement), conftest.rel_err for the states.  Every grid has at most 101 points.
"""
import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd.weights import init_term
from conftest import rel_err
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights import _fields
from test_path_weights_cpu import TAGS
from test_particle_filter_cpu import (BATCH_TIMES, FRACTIONS, OU_BIG, PLACEMENTS, QUIET, SEED, SEED_BATCH, batch_case, case, log_mean_exp,
                                      particle_filter_numpy, placement_case, reference)

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _prior(q):
    d = int(q.dim_d)
    return np.reshape(np.asarray(q.mu0, dtype=float), (1, d)), np.reshape(np.asarray(q.tau0, dtype=float), (1, d, d))


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _ctx(cache, tag):
    if tag not in cache:
        q = case(tag)[0]
        d = int(q.dim_d)
        cache[tag] = va.Context(q.model, getattr(q, "method", "euler"), d, int(q.n_pts), float(q.dt), sigma=np.reshape(np.asarray(q.sigma, dtype=float), (d, d)),
                                theta=np.atleast_1d(q.theta), m0=np.atleast_1d(q.m0), s0=np.reshape(np.asarray(q.s0, dtype=float), (d, d)),
                                obs_t=q.obs_t, obs_y=q.obs_y, obs_noise=np.reshape(np.asarray(q.obs_noise, dtype=float), (d, d)),
                                obs_h=None if getattr(q, "obs_h", None) is None else np.reshape(np.asarray(q.obs_h, dtype=float), (d, d)))
    return cache[tag]


def _compare(got, want, k=0, label=""):
    """row k of Context.particle_filter's dict against one restatement"""
    m, n = want["ess"].size, want["lw"].size
    assert np.array_equal(got["resampled"][k, :m], want["resampled"]), (label, got["resampled"][k], want["resampled"])
    assert np.array_equal(got["ancestors"][k, :m], want["ancestors"]), label
    worst = {"ess": float(np.max(np.abs(got["ess"][k, :m] - want["ess"]) / want["ess"])) if m else 0.0,
             "logw": float(np.max(np.abs(got["log_w"][k] - want["lw"]) / (1.0 + want["scale"]))),
             "state": rel_err(got["state"][k], want["state"]),
             "clouds": rel_err(got["clouds"][k, :m], want["clouds"]) if m else 0.0}
    print(label, "worst:", worst, " resampled:", want["resampled"])
    assert np.all(np.isfinite(got["log_w"][k])) and np.all(np.isfinite(got["state"][k]))
    assert max(worst.values()) <= TOL, (label, worst)
    # rows beyond the problem's own count
    assert np.all(got["ess"][k, m:] == 0.0) and np.all(got["resampled"][k, m:] == 0) and np.all(got["ancestors"][k, m:] == -1)
    assert np.all(np.isnan(got["clouds"][k, m:]))


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_it_is_the_weighted_sampler(contexts, tag, start):
    """ess_fraction = 0: the log-weights are sample_paths_weighted's path + obs + the host's init term, the final particles the last points of
    its paths, nothing is resampled"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    scale = particle_filter_numpy(q, x, s0, 17, SEED, 0.0)["scale"]
    got = ctx.particle_filter(17, SEED, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q), history=True)
    paths, logw, first = ctx.sample_paths_weighted(17, SEED, x=x, x0=s0)
    init = np.zeros(17) if start == "given" else init_term(first[0], q.mu0, q.tau0, q.m0, q.s0)
    worst = float(np.max(np.abs(got["log_w"][0] - (init + logw[0, :, 0] + logw[0, :, 1])) / (1.0 + scale)))
    last = rel_err(got["state"][0], paths[0, :, -1])
    print(tag, start, "worst |lw - (init + path + obs)| / (1 + scale) =", worst, " final state vs the sampler's last point: rel.err", last,
          " bit-equal:", bool(np.array_equal(got["state"][0], paths[0, :, -1])))
    assert worst <= TOL and last <= 1e-12
    assert not got["resampled"].any() and np.array_equal(got["ancestors"][0], np.tile(np.arange(17), (got["ess"].shape[1], 1)))
    assert np.all(got["ess"][0] >= 1.0 - 1e-12) and np.all(got["ess"][0] <= 17.0 + 1e-9)


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_against_numpy(contexts, tag, start, n_paths, ess_fraction):
    """one lane, a partial block of 64 paths, a second block, more than one 256-slot pass of the resampling kernel; collapsed clouds (the
    fixtures: one survivor) and the quiet cases' mix of resampled and carried clouds (started at 0, which defines them)"""
    q, x, x0 = case(tag)
    want = reference(tag, start, n_paths, ess_fraction)
    got = _ctx(contexts, tag).particle_filter(n_paths, SEED, ess_fraction=ess_fraction, x=x, x0=x0 if start == "given" else None,
                                              prior=_prior(q), history=True)
    _compare(got, want, label=f"{tag} n={n_paths} {start} f={ess_fraction}")
    if n_paths == 1:
        assert not got["resampled"].any()      # (ESS = 1 = n exactly)


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 weighs and resamples the start; adjacent indices; nothing is resampled at Np - 1"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        got = ctx.particle_filter(17, SEED, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q), history=True)
        want = particle_filter_numpy(q, x, x0, 17, SEED, 1.0)
        _compare(got, want, label=f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}")
        if obs_at[-1] == 40:
            assert got["resampled"][0, -1] == 0 and np.array_equal(got["ancestors"][0, -1], np.arange(17))
    ctx.close()


def _batch_context(model, d, probs):
    nb, n = 3, 41
    m = max(t.size for t in BATCH_TIMES)
    obs_t, obs_y = np.full((nb, m), -1, dtype=np.int64), np.full((nb, m, d), np.nan)
    for k, q in enumerate(probs):
        obs_t[k, :BATCH_TIMES[k].size], obs_y[k, :BATCH_TIMES[k].size] = BATCH_TIMES[k], q.obs_y
    p0 = probs[0]
    ctx = va.Context(model, "euler", d, n, p0.dt, sigma=p0.sigma, theta=np.atleast_1d(p0.theta), m0=p0.m0, s0=p0.s0, obs_t=p0.obs_t,
                     obs_y=p0.obs_y, obs_noise=p0.obs_noise, obs_h=p0.obs_h, batch=nb)
    ctx.set_problem_obs_model(n_obs=[t.size for t in BATCH_TIMES], obs_noise=np.stack([q.obs_noise for q in probs]),
                              obs_h=np.stack([q.obs_h for q in probs]))
    ctx.set_problem_data(obs_t=obs_t, obs_y=obs_y, m0=np.stack([q.m0 for q in probs]), s0=np.stack([q.s0 for q in probs]))
    ctx.set_problem_params(theta=np.stack([np.atleast_1d(q.theta) for q in probs]), sigma=np.stack([q.sigma for q in probs]))
    return ctx


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3: own observation times and counts (the cuts are the union; a problem without an observation at a cut is carried through), own
    theta, Sigma, prior moments, dense R and H; 40 particles: at D <= 4 the lanes of a wave belong to different problems.  The last
    problem's result is bit for bit the same beside two other neighbours."""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        runs[first] = ctx.particle_filter(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior, history=True)
        ctx.close()
        for k, q in enumerate(probs):
            _compare(runs[first], particle_filter_numpy(q, xs[k], None, 40, SEED_BATCH, 0.5, index=k), k=k, label=f"{model} batch {first} problem {k}")
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2], equal_nan=True), key
    assert not np.array_equal(runs[20]["log_w"][0], runs[50]["log_w"][0])


def test_many_particles_on_ou(contexts):
    tag, start, n, frac, seed = OU_BIG
    q, x, _ = case(tag)
    want = reference(*OU_BIG)
    got = _ctx(contexts, tag).particle_filter(n, seed, ess_fraction=frac, x=x, prior=_prior(q))
    assert got["ancestors"] is None and got["clouds"] is None
    ev, ev_ref = log_mean_exp(got["log_w"][0]), log_mean_exp(want["lw"])
    err_ess = float(np.max(np.abs(got["ess"][0] - want["ess"]) / want["ess"]))
    print("OU, 4096 particles: log-evidence", ev, "restatement", ev_ref, " ess", got["ess"][0], " rel.err of ess", err_ess,
          " resampled", got["resampled"][0])
    assert abs(ev - ev_ref) <= TOL * (1.0 + float(want["scale"].max())) and err_ess <= TOL
    assert np.array_equal(got["resampled"][0], want["resampled"]) and want["resampled"].any()


CACHE_CASES = [("L63", "rk4", None, 1.0, 65), ("L96", "rk4", 40, 0.5, 65), ("L96", "rk4", 12, 0.5, 1)]


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_filter(x=None) are bit for bit what they
    are without the call (the orders of test_path_weights.test_the_cache_is_not_touched: recording changes the state by itself)."""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_filter(9, 4, prior=prior, history=True) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "filter", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["filter", "record"])
    for key in ("log_w", "state", "ess", "resampled", "ancestors"):
        assert np.array_equal(res[key], res_c[key]), key
    assert np.all(np.isfinite(res["log_w"]))
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    k = nb - 1
    want = particle_filter_numpy(probs[k], xs[k], None, 9, 4, 0.5, index=k)
    assert not want["margins"] or min(want["margins"]) >= 1e-7, want["margins"]      # (the condition, for this case)
    _compare(res, want, k=k, label=f"{name} cached x, problem {k}")


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_filter(5, 1, x=xs, prior=(mu, tau), history=True)       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)                         # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_filter(5, 1)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_filter(0, 1, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_filter(bad, 1, x=xs)
    assert same(usable(), ref)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_filter(5, 1, ess_fraction=bad, x=xs)
    assert ctx.particle_filter(5, 1, ess_fraction=0.0, x=xs)["log_w"].shape == (3, 5)
    assert ctx.particle_filter(5, 1, ess_fraction=1.0, x=xs)["log_w"].shape == (3, 5)
    # through the C ABI itself: a null logw / state, one prior pointer without the other
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    call = lambda *a: ctx._lib.vgpa_particle_filter(ctx._h, xx.ctypes.data, None, 5, 1, 0.5, *a, None, None, None, None)      # noqa: E731
    assert call(None, None, None, st.ctypes.data) == -1 and call(None, None, lw.ctypes.data, None) == -1
    assert call(mu.ctypes.data, None, lw.ctypes.data, st.ctypes.data) == -1 and call(None, tau.ctypes.data, lw.ctypes.data, st.ctypes.data) == -1
    assert call(None, None, lw.ctypes.data, st.ctypes.data) == 0
    assert same(usable(), ref)
    # a prior covariance that is not positive definite: refused for a drawn start, not read for a given one
    bad_tau = tau.copy()
    bad_tau[1, 3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="problem 1"):
        ctx.particle_filter(5, 1, x=xs, prior=(mu, bad_tau))
    assert ctx.particle_filter(5, 1, x=xs, x0=np.zeros((3, 12)), prior=(mu, bad_tau))["state"].shape == (3, 5, 12)
    # a dense Sigma in force
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert same(usable(), ref)
    # an S0 row that is not positive definite: refused for a drawn start, not needed for a given one
    s0 = np.stack([np.reshape(q.s0, (12, 12)) for q in probs])
    s0[2, 5, 5] = -0.2
    ctx.set_problem_data(obs_y=np.stack([np.reshape(q.obs_y, (-1, 12)) for q in probs]), m0=np.stack([q.m0 for q in probs]), s0=s0)
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        usable()
    assert ctx.particle_filter(5, 1, x=xs, x0=np.zeros((3, 12)))["log_w"].shape == (3, 5)
    ctx.close()
    # no model: ValueError; a model without prior moments and observations (ODE-only): RuntimeError
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_filter(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_filter(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    # D > 64
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_filter(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_problem_batch_records_and_lineages():
    """ProblemBatch.particle_filter and VarGP.particle_filter: one record per member with its own prior, against the restatement of index
    p; every lineage point is a row of the device's own cloud at that observation"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.particle_filter(17, SEED_BATCH, x=x, history=True)
    plain = pb.particle_filter(17, SEED_BATCH, x=x)
    pb.close()
    assert len(recs) == len(plain) == 3
    for k, p in enumerate(ps):
        want = particle_filter_numpy(_fields(p["vgp"]), x[k], None, 17, SEED_BATCH, 0.5, index=k)
        assert not want["margins"] or min(want["margins"]) >= 1e-7, (k, want["margins"])      # (the condition, for these cases)
        rec = recs[k]
        assert isinstance(rec, va.ParticleFilterResult) and len(rec) == 17
        assert np.array_equal(rec.resampled, want["resampled"].astype(bool)) and np.array_equal(rec.ancestors, want["ancestors"])
        assert np.max(np.abs(rec.log_w - want["lw"]) / (1.0 + want["scale"])) <= TOL and rel_err(rec.state, want["state"]) <= TOL
        assert plain[k].ancestors is None and plain[k].clouds is None and np.array_equal(plain[k].log_w, rec.log_w)
        assert np.isfinite(rec.log_evidence()) and 1.0 <= rec.final_ess() <= 17.0 and rec.mean(rec.state).shape == (12,)
        lin = rec.lineages()
        m = rec.ess.size
        assert lin.shape == (17, m, 12) and rec.clouds.shape == (m, 17, 12)
        for j in range(m):
            for i in range(17):
                assert np.any(np.all(rec.clouds[j] == lin[i, j], axis=1)), (k, i, j)
        with pytest.raises(ValueError):
            plain[k].lineages()
    # one VarGP of the 1-D models: the last axis is dropped
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.particle_filter(33, 3, x=v.initialization(), history=True)
    v.invalidate()
    assert rec.state.shape == (33,) and rec.clouds.shape == (rec.ess.size, 33) and rec.lineages().shape == (33, rec.ess.size)
