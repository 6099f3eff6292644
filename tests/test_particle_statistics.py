"""
The path statistics of the particle filter's lineages on the GPU (vgpa_particle_statistics).

Reference: test_particle_statistics_cpu.particle_statistics_numpy, computed once per case and never written.  The runs are those of
tests/test_particle_filter.py, whose resampling margins test_particle_filter_cpu.test_margin_condition asserts >= 1e-7: the device's
ancestors are the restatement's, so `resampled` is compared exactly and the rows entry by entry, |got - want| <= 1e-9 (scale + tiny) with
scale the lineage's own sum of |increments| (the suite's TOL on the sum's own scale, as for the log-weights).  The walk itself -- logw,
state, ess, resampled -- is compared bit for bit with particle_filter.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights import _fields
from test_path_weights_cpu import FIXTURES, TAGS, _sigma_diag
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import (FRACTIONS, OU_BIG, PLACEMENTS, QUIET, SEED, SEED_BATCH, batch_case, case, placement_case)
from test_particle_filter_cpu import reference as filter_reference
from test_particle_statistics_cpu import model_phi, particle_statistics_numpy, reference, weighted_mean
from test_sample_paths_cpu import model_drift

pytestmark = pytest.mark.gpu

TOL = 1e-9
TINY = float(np.finfo(float).tiny)
WALK = ("log_w", "state", "ess", "resampled")


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _compare(got, want, k=0, label=""):
    """row k of Context.particle_statistics' dict (per_particle=True) against one restatement"""
    m = want["ess"].size
    assert np.array_equal(got["resampled"][k, :m], want["resampled"]), (label, got["resampled"][k], want["resampled"])
    rows = got["stats"][k]
    assert rows.shape == want["rows"].shape and np.all(np.isfinite(rows)) and np.all(np.isfinite(got["mean"][k]))
    excess = np.abs(rows - want["rows"]) / (want["scale"] + TINY)
    worst = [float(excess[:, s].max()) for s in range(3)]
    host = weighted_mean(got["log_w"][k], rows)
    mean_err = float(np.max(np.abs(got["mean"][k] - host) / np.abs(host)))
    print(label, "worst |rows - want| / scale per statistic (Q, G, H):", worst, " device mean vs host mean of its rows: rel.err", mean_err,
          " resampled:", want["resampled"])
    assert max(worst) <= TOL, (label, worst)
    assert mean_err <= 1e-12, (label, mean_err)


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_against_numpy(contexts, tag, start, n_paths, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 5, 64 (NT = 16, 32, 48, 64; 17 odd; 64 without a padding row); one lane, a partial 16-path tile inside a
    partial block, a second workgroup of one path, more than one 256-slot pass of the resampling kernel; collapsed clouds (the fixtures:
    every row copied from one survivor) and the quiet cases' mix of copied and carried rows"""
    q, x, x0 = case(tag)
    want = reference(tag, start, n_paths, ess_fraction)
    walk = filter_reference(tag, start, n_paths, ess_fraction)
    assert np.array_equal(want["lw"], walk["lw"]) and np.array_equal(want["state"], walk["state"])      # (the restatements walk alike)
    got = _ctx(contexts, tag).particle_statistics(n_paths, SEED, ess_fraction=ess_fraction, x=x, x0=x0 if start == "given" else None,
                                                  prior=_prior(q), per_particle=True)
    _compare(got, want, label=f"{tag} n={n_paths} {start} f={ess_fraction}")


def test_the_parametrisation_copies_and_carries_rows():
    """a condition on the cases: the fixtures collapse to one survivor, the quiet cases resample at some observations and not at others"""
    assert any(reference(t, "given", 65, 0.5)["resampled"].any() for t in FIXTURES)
    kinds = set()
    for t in QUIET:
        kinds |= set(reference(t, "given", 65, 0.5)["resampled"][:-1].tolist())
    assert kinds == {0, 1}


@pytest.mark.parametrize("tag", TAGS + QUIET)
def test_the_walk_is_the_filters(contexts, tag):
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    for start in ((x0,) if tag in QUIET else (x0, None)):
        got = ctx.particle_statistics(65, SEED, ess_fraction=0.5, x=x, x0=start, prior=_prior(q), per_particle=True)
        flt = ctx.particle_filter(65, SEED, ess_fraction=0.5, x=x, x0=start, prior=_prior(q))
        for key in WALK:
            assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (tag, key)


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_devices_stored_paths(contexts, tag, start):
    """ess_fraction = 0: the rows are the statistics of the paths sample_paths_weighted stores for the same seed, recomputed on the host"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    scale = reference(tag, start, 17, 0.0)["scale"]
    got = ctx.particle_statistics(17, SEED, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q), per_particle=True)
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=s0)[0][0]
    dt, theta = float(q.dt), np.asarray(q.theta, dtype=float)
    want = np.zeros((17, 3, int(q.dim_d)))
    for k in range(1, int(q.n_pts)):
        prev = paths[:, k - 1]
        res, phi = (paths[:, k] - prev) - dt * model_drift(q.model, theta, prev), model_phi(q.model, prev)
        want += np.stack((res * res / dt, phi * res, dt * (phi * phi)), axis=1)
    worst = float(np.max(np.abs(got["stats"][0] - want) / (scale + TINY)))
    print(tag, start, "worst |rows - statistics of the stored paths| / scale =", worst)
    assert worst <= TOL and not got["resampled"].any()


@pytest.mark.parametrize("which", ["n300", "ou_big"])
def test_device_mean(contexts, which):
    """the mean reduced on the device against the host's weighted mean of the device's own rows; the mean alone (no rows downloaded)"""
    tag, start, n, frac, seed = ("l96d40_rk4_p", "drawn", 300, 0.5, SEED) if which == "n300" else OU_BIG
    q, x, _ = case(tag)
    ctx = _ctx(contexts, tag)
    both = ctx.particle_statistics(n, seed, ess_fraction=frac, x=x, prior=_prior(q), per_particle=True)
    alone = ctx.particle_statistics(n, seed, ess_fraction=frac, x=x, prior=_prior(q))
    host = weighted_mean(both["log_w"][0], both["stats"][0])
    err = float(np.max(np.abs(both["mean"][0] - host) / np.abs(host)))
    print(which, "device mean vs host mean: rel.err", err, " E[G]", both["mean"][0, 1].ravel()[:3])
    assert err <= 1e-12
    assert alone["stats"] is None and np.array_equal(alone["mean"], both["mean"])
    for key in WALK:
        assert np.array_equal(alone[key], both[key]), key
    if which == "ou_big":
        want = reference(*OU_BIG)
        assert np.array_equal(both["resampled"][0], want["resampled"]) and want["resampled"].any()
        assert float(np.max(np.abs(both["stats"][0] - want["rows"]) / (want["scale"] + TINY))) <= TOL


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (an empty first segment), adjacent indices (segments of one step), Np - 1"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        got = ctx.particle_statistics(17, SEED, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q), per_particle=True)
        _compare(got, particle_statistics_numpy(q, x, x0, 17, SEED, 1.0), label=f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}")
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_no_observations(model, d):
    """a context without observations: one segment, no resampling step; the rows are those of ess_fraction = 0"""
    q, x = placement_case(model, d, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, d)))
    ctx = va.Context(model, "euler", d, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    got = ctx.particle_statistics(17, SEED, ess_fraction=0.5, x=x, x0=x0, per_particle=True)
    zero = ctx.particle_statistics(17, SEED, ess_fraction=0.0, x=x, x0=x0, per_particle=True)
    ctx.close()
    assert got["ess"].shape == (1, 0) and np.array_equal(got["stats"], zero["stats"]) and np.array_equal(got["mean"], zero["mean"])
    _compare(got, particle_statistics_numpy(q, x, x0, 17, SEED, 0.5), label=f"{model} no observations")


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with own theta, isotropic Sigma, observation times, counts, R and H: row k is the single-problem restatement of index k, and the
    last problem's result is bit for bit the same beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        runs[first] = ctx.particle_statistics(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior, per_particle=True)
        flt = ctx.particle_filter(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        ctx.close()
        for key in WALK:
            assert np.array_equal(runs[first][key], flt[key]), key
        for k, q in enumerate(probs):
            _compare(runs[first], particle_statistics_numpy(q, xs[k], None, 40, SEED_BATCH, 0.5, index=k), k=k,
                     label=f"{model} batch {first} problem {k}")
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["stats"][0], runs[50]["stats"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_statistics(x=None) are bit for bit what
    they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_statistics(9, 4, prior=prior, per_particle=True) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "statistics", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["statistics", "record"])
    for key in WALK + ("stats", "mean"):
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    k = nb - 1
    want = particle_statistics_numpy(probs[k], xs[k], None, 9, 4, 0.5, index=k)
    assert not want["margins"] or min(want["margins"]) >= 1e-7, want["margins"]      # (the condition, for this case)
    _compare(res, want, k=k, label=f"{name} cached x, problem {k}")


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_statistics(5, 1, x=xs, prior=(mu, tau), per_particle=True)       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)                                # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_statistics(5, 1)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_statistics(0, 1, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_statistics(bad, 1, x=xs)
    assert same(usable(), ref)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_statistics(5, 1, ess_fraction=bad, x=xs)
    # through the C ABI itself: both outputs null; one of them is enough
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    rows, mean = np.empty((3, 5, 3, 12)), np.empty((3, 3, 12))
    call = lambda a, b: ctx._lib.vgpa_particle_statistics(ctx._h, xx.ctypes.data, None, 5, 1, 0.5, None, None, lw.ctypes.data, st.ctypes.data,      # noqa: E731
                                                          a, b, None, None)
    assert call(None, None) == -1 and b"stats and mean" in ctx._lib.vgpa_last_error(ctx._h)
    assert call(rows.ctypes.data, None) == 0 and call(None, mean.ctypes.data) == 0
    assert same(usable(), ref)
    # a dense Sigma in force
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert same(usable(), ref)
    ctx.close()
    # no model: ValueError; D > 64: NotImplementedError, and the context stays usable
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_statistics(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_statistics(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_particle_fit_theta_on_ou():
    """two iterations at fixed (A_t, b_t): the theta trace is the one the restatement's statistics give with the same seeds; the records of
    VarGP and ProblemBatch"""
    v = build_problem("OU", "euler", 0.5)["vgp"]
    x = v.initialization()
    q = _fields(v)
    theta0, sg = float(q.theta), _sigma_diag(q).diagonal()
    rec = v.particle_statistics(300, 11, x=x, per_particle=True)
    assert isinstance(rec, va.PathStatistics) and len(rec) == 300 and rec.rows.shape == (300, 3, 1) and rec.model == "OU"
    assert rec.n_steps == v.dim_n - 1 and rec.dt == float(v.fwd_ode.dt)
    want = [theta0]
    for it in range(2):
        ref = particle_statistics_numpy(q, x, None, 300, 11 + it, 0.5)
        assert not ref["margins"] or min(ref["margins"]) >= 1e-7, ref["margins"]      # (the condition, for these runs)
        mean = weighted_mean(ref["lw"], ref["rows"])
        if it == 0:
            assert np.max(np.abs(rec.mean - mean) / np.abs(mean)) <= 1e-8
        q.theta = q.theta + float(np.sum(mean[1] / sg) / np.sum(mean[2] / sg))
        want.append(q.theta)
    pb = va.ProblemBatch([v])
    theta, trace = pb.particle_fit_theta(300, 11, 2, refit=False, x0=x)
    pb.close()
    print("theta trace", trace["theta"].ravel(), "restatement", want, "log-evidence", trace["log_evidence"].ravel())
    assert trace["theta"].shape == (3, 1, 1) and trace["log_evidence"].shape == (2, 1) and np.all(np.isfinite(trace["log_evidence"]))
    assert np.max(np.abs(trace["theta"].ravel() - np.array(want))) <= 1e-8
    assert float(v.model.theta) == float(theta[0, 0]) == trace["theta"][-1, 0, 0] and theta[0, 0] != theta0
    # the default: (A_t, b_t) refitted at every theta; the statistics are the restatement's at the x each step used
    v.model.theta = theta0
    got, tr = v.particle_fit_theta(300, 11, 1)
    v.invalidate()
    q.theta = theta0
    ref = particle_statistics_numpy(q, tr["x"][0, 0], None, 300, 11, 0.5)
    assert not ref["margins"] or min(ref["margins"]) >= 1e-7, ref["margins"]
    mean = weighted_mean(ref["lw"], ref["rows"])
    assert abs(got - (theta0 + float(np.sum(mean[1] / sg) / np.sum(mean[2] / sg)))) <= 1e-8 and isinstance(got, float)
