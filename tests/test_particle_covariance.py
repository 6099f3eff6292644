"""
The smoothing mean and full second-moment matrices on the grid under the particle filter's genealogy on the GPU (vgpa_particle_covariance).

Reference: test_particle_covariance_cpu.particle_covariance_numpy (every slot carries its whole path: the forward algorithm), computed once
per case and never written.  The runs are those of tests/test_particle_moments.py and tests/test_particle_filter.py, whose resampling
margins test_particle_filter_cpu.test_margin_condition and test_particle_moments_cpu.test_margin_condition_of_the_runs_not_cleared_elsewhere
assert >= 1e-7: the device's ancestors are the restatement's.  The walk itself -- logw, state (copied behind the replay), ess, resampled --
is compared bit for bit with particle_filter, lineage_ess bit for bit with particle_moments; the sums with the suite's 1e-9 on their own
scales, computed by the restatement:
    |mean - m1| <= 1e-9 sum_i W_i |x_i|,   |second - want| <= 1e-9 sum_i W_i |x_i[a]| |x_i[b]| + tiny,   |diag(second) - M2| <= 1e-9 M2
with M2 of particle_moments, and second[k] equal to its transpose to the bit.  Every grid has at most 101 points.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights import _fields
from test_path_weights_cpu import TAGS
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import (FRACTIONS, OU_BIG, PLACEMENTS, QUIET, SEED, SEED_BATCH, batch_case, case, placement_case)
from test_particle_covariance_cpu import particle_covariance_numpy, reference, weighted_second

pytestmark = pytest.mark.gpu

TOL = 1e-9
TINY = float(np.finfo(float).tiny)
WALK = ("log_w", "state", "ess", "resampled")
WORST = {"mean": 0.0, "second": 0.0, "diagonal": 0.0}      # over the module, printed by the last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _compare(got, want, stride, k=0, label="", moments=None):
    """row k of Context.particle_covariance's dict against one restatement, on the grid indices 0, stride, ...; moments: the dict of
    Context.particle_moments with the same arguments"""
    m = want["ess"].size
    assert np.array_equal(got["resampled"][k, :m], want["resampled"]), (label, got["resampled"][k], want["resampled"])
    mean, sec = got["mean"][k], got["second"][k]
    m1, a1, s2, a2 = want["m1"][::stride], want["a1"][::stride], want["second"][::stride], want["a2"][::stride]
    assert mean.shape == m1.shape and sec.shape == s2.shape and np.all(np.isfinite(mean)) and np.all(np.isfinite(sec))
    assert np.array_equal(sec, np.transpose(sec, (0, 2, 1))), label
    e1, e2 = np.abs(mean - m1), np.abs(sec - s2)
    worst = {"mean": float(np.max(e1 / (a1 + TINY))), "second": float(np.max(e2 / (a2 + TINY)))}
    if moments is not None:
        big = moments["moments"][k, :, 1]
        ed = np.abs(np.diagonal(sec, axis1=1, axis2=2) - big)
        worst["diagonal"] = float(np.max(ed / (big + TINY)))
        assert np.array_equal(got["lineage_ess"][k], moments["lineage_ess"][k]), label
    print(label, f"stride {stride} worst:", worst, " resampled:", want["resampled"])
    for key, val in worst.items():
        WORST[key] = max(WORST[key], val)
    assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * a2 + TINY), (label, worst)
    if moments is not None:
        assert np.all(ed <= TOL * big), (label, worst)
    assert np.all(got["lineage_ess"][k, m + 1:] == 0.0)      # rows beyond the problem's own count + 1


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_against_numpy(contexts, tag, start, n_paths, ess_fraction):
    """The cases of test_particle_moments.test_against_numpy.  D = 1, 1, 3 (the lane kernel; off-diagonal entries at 3 and 4), 5 (NT = 16),
    12, 17 (NT = 32: padded rows inside a tile), 40 (NT = 48: six tiles in two rounds), 64 (NT = 64: ten tiles in three rounds, no padding
    row); one lane, a partial 16-path tile (weight-0 lanes in the product), a second workgroup that holds one path, several workgroups;
    every grid index, every fourth and index 0 alone.  The walk is the filter's, bit for bit, lineage_ess the moments', the strided
    results are the stride-1 result's rows, and a second call gives the same bits."""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    want = reference(tag, start, n_paths, ess_fraction)
    s0 = x0 if start == "given" else None
    flt = ctx.particle_filter(n_paths, SEED, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    for stride in (1, 4, int(q.n_pts) + 3):
        got = ctx.particle_covariance(n_paths, SEED, stride=stride, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
        mom = ctx.particle_moments(n_paths, SEED, stride=stride, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
        for key in WALK:
            assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (tag, stride, key)
        _compare(got, want, stride, label=f"{tag} n={n_paths} {start} f={ess_fraction}", moments=mom)
        if stride == 1:
            first = got
        else:
            assert got["second"].shape[1] == (int(q.n_pts) - 1) // stride + 1
            assert np.array_equal(got["second"][0], first["second"][0, ::stride]) and np.array_equal(got["mean"][0], first["mean"][0, ::stride])
            assert np.array_equal(got["lineage_ess"], first["lineage_ess"])
    again = ctx.particle_covariance(n_paths, SEED, stride=1, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    for key in first:
        assert np.array_equal(again[key], first[key]), key


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_devices_stored_paths(contexts, tag, start):
    """ess_fraction = 0: the matrices are the device's own sample_paths_weighted paths reweighted on the host with the call's own final
    weights (every W row is the final one, the states are the sampler's)"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    got = ctx.particle_covariance(17, SEED, stride=1, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q))
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=s0)[0][0]
    w = np.exp(got["log_w"][0] - got["log_w"][0].max())
    w = w / w.sum()
    m1, a1 = np.einsum("i,ikd->kd", w, paths), np.einsum("i,ikd->kd", w, np.abs(paths))
    s2, a2 = weighted_second(w, paths), weighted_second(w, np.abs(paths))
    e1, e2 = np.abs(got["mean"][0] - m1), np.abs(got["second"][0] - s2)
    print(tag, start, "worst against the reweighted stored paths:", float(np.max(e1 / (a1 + TINY))), float(np.max(e2 / (a2 + TINY))))
    assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * a2 + TINY) and not got["resampled"].any()
    assert np.allclose(got["lineage_ess"][0], 1.0 / np.sum(w * w), rtol=TOL)


def test_many_particles_on_ou(contexts):
    """the one larger run: 16 workgroups of the small kernel, 16 passes of the descendant sums, two resamplings"""
    tag, start, n, frac, seed = OU_BIG
    q, x, _ = case(tag)
    ctx = _ctx(contexts, tag)
    want = reference(*OU_BIG)
    got = ctx.particle_covariance(n, seed, stride=1, ess_fraction=frac, x=x, prior=_prior(q))
    flt = ctx.particle_filter(n, seed, ess_fraction=frac, x=x, prior=_prior(q))
    mom = ctx.particle_moments(n, seed, stride=1, ess_fraction=frac, x=x, prior=_prior(q))
    for key in WALK:
        assert np.array_equal(got[key], flt[key]), key
    assert want["resampled"].any()
    _compare(got, want, 1, label="OU, 4096 particles", moments=mom)
    again = ctx.particle_covariance(n, seed, stride=1, ess_fraction=frac, x=x, prior=_prior(q))
    assert np.array_equal(again["second"], got["second"]) and np.array_equal(again["mean"], got["mean"])


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (an empty first segment that reduces index 0 with stretch 0's weights), adjacent indices (segments
    of one step), Np - 1 (an empty last stretch)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        want = particle_covariance_numpy(q, x, x0, 17, SEED, 1.0)
        flt = ctx.particle_filter(17, SEED, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
        for stride in (1, 4):
            got = ctx.particle_covariance(17, SEED, stride=stride, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
            mom = ctx.particle_moments(17, SEED, stride=stride, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
            for key in WALK:
                assert np.array_equal(got[key], flt[key]), key
            _compare(got, want, stride, label=f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}", moments=mom)
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_no_observations(model, d):
    """a context without observations: one segment, one stretch, the final weights (all equal for a given start)"""
    q, x = placement_case(model, d, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, d)))
    ctx = va.Context(model, "euler", d, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    got = ctx.particle_covariance(17, SEED, ess_fraction=0.5, x=x, x0=x0)
    flt = ctx.particle_filter(17, SEED, ess_fraction=0.5, x=x, x0=x0)
    mom = ctx.particle_moments(17, SEED, ess_fraction=0.5, x=x, x0=x0)
    ctx.close()
    assert got["ess"].shape == (1, 0) and got["lineage_ess"].shape == (1, 1)
    for key in WALK:
        assert np.array_equal(got[key], flt[key]), key
    _compare(got, particle_covariance_numpy(q, x, x0, 17, SEED, 0.5), 1, label=f"{model} no observations", moments=mom)


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with own theta, isotropic Sigma, observation times, counts, R and H: a cut of the batch lies inside a stretch of a problem
    without an observation there; row k is the single-problem restatement of index k, and the last problem's result is bit for bit the
    same beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        runs[first] = ctx.particle_covariance(40, SEED_BATCH, stride=1, ess_fraction=0.5, x=xs, prior=prior)
        third = ctx.particle_covariance(40, SEED_BATCH, stride=3, ess_fraction=0.5, x=xs, prior=prior)
        flt = ctx.particle_filter(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        mom = ctx.particle_moments(40, SEED_BATCH, stride=1, ess_fraction=0.5, x=xs, prior=prior)
        ctx.close()
        for key in WALK:
            assert np.array_equal(runs[first][key], flt[key]) and np.array_equal(third[key], flt[key]), key
        assert np.array_equal(third["second"], runs[first]["second"][:, ::3]) and np.array_equal(third["mean"], runs[first]["mean"][:, ::3])
        for k, q in enumerate(probs):
            _compare(runs[first], particle_covariance_numpy(q, xs[k], None, 40, SEED_BATCH, 0.5, index=k), 1, k=k,
                     label=f"{model} batch {first} problem {k}", moments=mom)
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["second"][0], runs[50]["second"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_covariance(x=None) are bit for bit what
    they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_covariance(9, 4, prior=prior) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "covariance", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["covariance", "record"])
    for key in WALK + ("mean", "second", "lineage_ess"):
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    k = nb - 1
    want = particle_covariance_numpy(probs[k], xs[k], None, 9, 4, 0.5, index=k)
    assert not want["margins"] or min(want["margins"]) >= 1e-7, want["margins"]      # (the condition, for this case)
    _compare(res, want, 1, k=k, label=f"{name} cached x, problem {k}")


def test_errors():
    """The error codes of particle_moments, a NULL mean or second, and the workgroup limit refused before any work with the cache intact.
    (The other limit, 2^39 - 256 entries of `second`, needs batch * Np >= 2^27 at D = 64: a context of terabytes; the host checks it in the
    same place, before the workgroup limit's neighbour.)"""
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_covariance(5, 1, x=xs, prior=(mu, tau))       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)             # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_covariance(5, 1)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_covariance(0, 1, x=xs)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_covariance(5, 1, stride=bad, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_covariance(5, 1, stride=bad, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_covariance(bad, 1, x=xs)
    big_stride = ctx.particle_covariance(5, 1, stride=2 ** 31 - 1, x=xs)
    assert big_stride["second"].shape == (3, 1, 12, 12) and big_stride["mean"].shape == (3, 1, 12)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_covariance(5, 1, ess_fraction=bad, x=xs)
    # the limits, refused before any work with the cache intact: more workgroups per problem than a launch holds ...
    ctx.free_energy(xs)
    before = [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st"))]
    with pytest.raises(NotImplementedError, match="particles per problem"):
        ctx.particle_covariance(65535 * 64 + 1, 1, x=xs)
    with pytest.raises(NotImplementedError, match="particles per problem"):
        ctx.particle_covariance(65535 * 64 + 1, 1)
    after = [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st"))]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # through the C ABI itself: a null mean, second, logw or state; lineage_ess, ess and resampled are optional
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    mean, sec = np.empty((3, ctx.Np, 12)), np.empty((3, ctx.Np, 12, 12))
    call = lambda a, b, c, d: ctx._lib.vgpa_particle_covariance(ctx._h, xx.ctypes.data, None, 5, 1, 1, 0.5, None, None, a, b, c, d, None, None, None)      # noqa: E731
    assert call(lw.ctypes.data, st.ctypes.data, None, sec.ctypes.data) == -1 and call(lw.ctypes.data, st.ctypes.data, mean.ctypes.data, None) == -1
    assert call(None, st.ctypes.data, mean.ctypes.data, sec.ctypes.data) == -1 and call(lw.ctypes.data, None, mean.ctypes.data, sec.ctypes.data) == -1
    assert call(lw.ctypes.data, st.ctypes.data, mean.ctypes.data, sec.ctypes.data) == 0
    res = ctx.particle_covariance(5, 1, x=xs)
    assert np.array_equal(sec, res["second"]) and np.array_equal(mean, res["mean"])
    assert same(usable(), ref)
    # a dense Sigma in force
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert same(usable(), ref)
    ctx.close()
    # no model: ValueError; ODE-only: RuntimeError; D > 64: NotImplementedError, and the context stays usable
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_covariance(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_covariance(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_covariance(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records_of_vargp_and_problem_batch():
    """ProblemBatch.particle_covariance and VarGP.particle_covariance: one SmoothingCovariance per member, equal to the bare context's rows
    and to the restatement of index p; the 1-D models drop the component axes"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.particle_covariance(17, SEED_BATCH, stride=2, x=x)
    d = 12
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(3, d, d))
    bare = pb._context().particle_covariance(17, SEED_BATCH, stride=2, x=pb._stack(x), prior=prior)
    pb.close()
    assert len(recs) == 3
    for k, p in enumerate(ps):
        want = particle_covariance_numpy(_fields(p["vgp"]), x[k], None, 17, SEED_BATCH, 0.5, index=k)
        assert not want["margins"] or min(want["margins"]) >= 1e-7, (k, want["margins"])      # (the condition, for these cases)
        rec = recs[k]
        assert isinstance(rec, va.SmoothingCovariance) and len(rec) == 17 and rec.stride == 2
        assert np.array_equal(rec.mean, bare["mean"][k]) and np.array_equal(rec.second, bare["second"][k]) and np.array_equal(rec.log_w, bare["log_w"][k])
        cov = bare["second"][k] - bare["mean"][k][:, :, None] * bare["mean"][k][:, None, :]
        assert np.array_equal(rec.cov, cov) and np.array_equal(rec.var, np.diagonal(cov, axis1=1, axis2=2))
        assert np.array_equal(rec.grid, np.arange(0, int(want["m1"].shape[0]), 2))
        assert np.array_equal(rec.lineage_ess, bare["lineage_ess"][k, :rec.obs_t.size + 1]) and np.array_equal(rec.obs_t, want["obs_t"])
        assert rec.lineage_ess_on_grid().shape == rec.grid.shape and np.isfinite(rec.log_evidence())
        last = int(rec.grid[-1])
        g_mean, g_cov = rec.gaussian(last)
        assert np.array_equal(g_mean, rec.mean[-1]) and np.array_equal(g_cov, rec.cov[-1]) and np.array_equal(g_cov, g_cov.T)
        with pytest.raises(ValueError):
            rec.gaussian(1)
        _compare(bare, want, 2, k=k, label=f"ProblemBatch member {k}")
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.particle_covariance(33, 3, x=v.initialization())
    v.invalidate()
    assert rec.mean.shape == rec.var.shape == rec.cov.shape == rec.second.shape == (v.dim_n,) and rec.lineage_ess.size == rec.obs_t.size + 1
    assert rec.lineage_ess_on_grid()[-1] == rec.lineage_ess[np.searchsorted(rec.obs_t, v.dim_n - 1)]
    assert np.ndim(rec.gaussian(v.dim_n - 1)[1]) == 0


def test_report_worst_deviations():
    """No check of its own: prints the largest deviations the comparisons of this module have seen in this process so far (run behind
    them, the figures DESIGN.md s.4.16 quotes); every comparison asserts its own bound in _compare."""
    print("worst deviations over the module, in units of their scales:", WORST)
