"""
The smoothing moments on the grid under the particle filter's genealogy on the GPU (vgpa_particle_moments).

Reference: test_particle_moments_cpu.particle_moments_numpy (every slot carries its whole path: the forward algorithm), computed once per
case and never written.  The runs are those of tests/test_particle_filter.py, whose resampling margins
test_particle_filter_cpu.test_margin_condition asserts >= 1e-7 (the others assert the condition where they are made): the device's
ancestors are the restatement's.  The walk itself -- logw, state (copied behind the replay), ess, resampled -- is compared bit for bit with
particle_filter; the moments with the suite's 1e-9 on the sums' own scales, computed by the restatement:
    |M1 - want| <= 1e-9 sum_i W_i |x_i|,   |M2 - want| <= 1e-9 M2,   lineage_ess to 1e-9 relative.
Every grid has at most 101 points.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights import _fields
from test_path_weights_cpu import FIXTURES, TAGS
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import (FRACTIONS, OU_BIG, PLACEMENTS, QUIET, SEED, SEED_BATCH, batch_case, case, placement_case)
from test_particle_moments_cpu import particle_moments_numpy, reference

pytestmark = pytest.mark.gpu

TOL = 1e-9
WALK = ("log_w", "state", "ess", "resampled")
WORST = {"m1": 0.0, "m2": 0.0, "lineage_ess": 0.0}      # over the module, printed by the last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _compare(got, want, stride, k=0, label=""):
    """row k of Context.particle_moments' dict against one restatement, on the grid indices 0, stride, ..."""
    m = want["ess"].size
    assert np.array_equal(got["resampled"][k, :m], want["resampled"]), (label, got["resampled"][k], want["resampled"])
    mom = got["moments"][k]
    m1, m2, a1 = want["m1"][::stride], want["m2"][::stride], want["a1"][::stride]
    assert mom.shape == (m1.shape[0], 2, m1.shape[1]) and np.all(np.isfinite(mom))
    e1, e2 = np.abs(mom[:, 0] - m1), np.abs(mom[:, 1] - m2)
    tiny = float(np.finfo(float).tiny)
    worst = {"m1": float(np.max(e1 / (a1 + tiny))), "m2": float(np.max(e2 / (m2 + tiny))),
             "lineage_ess": float(np.max(np.abs(got["lineage_ess"][k, :m + 1] - want["lineage_ess"]) / want["lineage_ess"]))}
    print(label, f"stride {stride} worst:", worst, " lineage ESS:", np.round(want["lineage_ess"], 2), " resampled:", want["resampled"])
    for key, val in worst.items():
        WORST[key] = max(WORST[key], val)
    assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * m2), (label, worst)
    assert worst["lineage_ess"] <= TOL, (label, worst)
    assert np.all(got["lineage_ess"][k, m + 1:] == 0.0)      # rows beyond the problem's own count + 1


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_against_numpy(contexts, tag, start, n_paths, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 5, 64 (NT = 16, 32, 48, 64; 17 odd; 64 without a padding row); one lane, a partial 16-path tile inside a
    partial block, a second workgroup, a second 256-slot workgroup at D <= 4 and a second pass of the descendant sums; collapsed clouds
    (the fixtures: one lineage carries the early stretches) and the quiet cases' mix of gathered and carried clouds; every grid index,
    every fourth (a segment without a kept index, kept indices on and off the cuts) and index 0 alone.  The walk is the filter's, bit for
    bit, and a second call gives the same bits."""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    want = reference(tag, start, n_paths, ess_fraction)
    s0 = x0 if start == "given" else None
    flt = ctx.particle_filter(n_paths, SEED, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    for stride in (1, 4, int(q.n_pts) + 3):
        got = ctx.particle_moments(n_paths, SEED, stride=stride, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
        for key in WALK:
            assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (tag, stride, key)
        _compare(got, want, stride, label=f"{tag} n={n_paths} {start} f={ess_fraction}")
        if stride == 1:
            first = got
        else:
            assert got["moments"].shape[1] == (int(q.n_pts) - 1) // stride + 1
            assert np.array_equal(got["moments"][0], first["moments"][0, ::stride]) and np.array_equal(got["lineage_ess"], first["lineage_ess"])
    again = ctx.particle_moments(n_paths, SEED, stride=1, ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    for key in first:
        assert np.array_equal(again[key], first[key]), key


def test_the_parametrisation_gathers_and_carries():
    """a condition on the cases: the fixtures collapse (an early stretch on one lineage), the quiet cases resample at some observations and
    not at others and keep several lineages"""
    assert any(reference(t, "given", 65, 0.5)["resampled"].any() and reference(t, "given", 65, 0.5)["lineage_ess"][0] < 1.5 for t in FIXTURES)
    kinds, most = set(), 0.0
    for t in QUIET:
        ref = reference(t, "given", 65, 0.5)
        kinds |= set(ref["resampled"][:-1].tolist())
        most = max(most, float(ref["lineage_ess"][0]))
    assert kinds == {0, 1} and most > 2.0


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_devices_stored_paths(contexts, tag, start):
    """ess_fraction = 0: the moments are the device's own sample_paths_weighted paths reweighted on the host with the call's own final
    weights (every W row is the final one, the states are the sampler's)"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    got = ctx.particle_moments(17, SEED, stride=1, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q))
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=s0)[0][0]
    w = np.exp(got["log_w"][0] - got["log_w"][0].max())
    w = w / w.sum()
    m1, m2, a1 = np.einsum("i,ikd->kd", w, paths), np.einsum("i,ikd->kd", w, paths * paths), np.einsum("i,ikd->kd", w, np.abs(paths))
    e1, e2 = np.abs(got["moments"][0, :, 0] - m1), np.abs(got["moments"][0, :, 1] - m2)
    print(tag, start, "worst against the reweighted stored paths:", float(np.max(e1 / (a1 + 1e-300))), float(np.max(e2 / (m2 + 1e-300))))
    assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * m2) and not got["resampled"].any()
    assert np.allclose(got["lineage_ess"][0], 1.0 / np.sum(w * w), rtol=TOL)


def test_many_particles_on_ou(contexts):
    """the one larger run: 16 workgroups of the small kernel, 16 passes of the descendant sums, two resamplings"""
    tag, start, n, frac, seed = OU_BIG
    q, x, _ = case(tag)
    ctx = _ctx(contexts, tag)
    want = reference(*OU_BIG)
    got = ctx.particle_moments(n, seed, stride=1, ess_fraction=frac, x=x, prior=_prior(q))
    flt = ctx.particle_filter(n, seed, ess_fraction=frac, x=x, prior=_prior(q))
    for key in WALK:
        assert np.array_equal(got[key], flt[key]), key
    assert want["resampled"].any()
    _compare(got, want, 1, label="OU, 4096 particles")
    again = ctx.particle_moments(n, seed, stride=1, ess_fraction=frac, x=x, prior=_prior(q))
    assert np.array_equal(again["moments"], got["moments"])


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (an empty first segment that reduces index 0 with stretch 0's weights), adjacent indices (segments
    of one step), Np - 1 (an empty last stretch)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        want = particle_moments_numpy(q, x, x0, 17, SEED, 1.0)
        flt = ctx.particle_filter(17, SEED, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
        for stride in (1, 4):
            got = ctx.particle_moments(17, SEED, stride=stride, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
            for key in WALK:
                assert np.array_equal(got[key], flt[key]), key
            _compare(got, want, stride, label=f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}")
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_no_observations(model, d):
    """a context without observations: one segment, one stretch, the final weights (all equal for a given start)"""
    q, x = placement_case(model, d, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, d)))
    ctx = va.Context(model, "euler", d, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    got = ctx.particle_moments(17, SEED, ess_fraction=0.5, x=x, x0=x0)
    flt = ctx.particle_filter(17, SEED, ess_fraction=0.5, x=x, x0=x0)
    ctx.close()
    assert got["ess"].shape == (1, 0) and got["lineage_ess"].shape == (1, 1)
    for key in WALK:
        assert np.array_equal(got[key], flt[key]), key
    _compare(got, particle_moments_numpy(q, x, x0, 17, SEED, 0.5), 1, label=f"{model} no observations")


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
        runs[first] = ctx.particle_moments(40, SEED_BATCH, stride=1, ess_fraction=0.5, x=xs, prior=prior)
        third = ctx.particle_moments(40, SEED_BATCH, stride=3, ess_fraction=0.5, x=xs, prior=prior)
        flt = ctx.particle_filter(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        ctx.close()
        for key in WALK:
            assert np.array_equal(runs[first][key], flt[key]) and np.array_equal(third[key], flt[key]), key
        assert np.array_equal(third["moments"], runs[first]["moments"][:, ::3])
        for k, q in enumerate(probs):
            _compare(runs[first], particle_moments_numpy(q, xs[k], None, 40, SEED_BATCH, 0.5, index=k), 1, k=k,
                     label=f"{model} batch {first} problem {k}")
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["moments"][0], runs[50]["moments"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_moments(x=None) are bit for bit what
    they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_moments(9, 4, prior=prior) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "moments", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["moments", "record"])
    for key in WALK + ("moments", "lineage_ess"):
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    k = nb - 1
    want = particle_moments_numpy(probs[k], xs[k], None, 9, 4, 0.5, index=k)
    assert not want["margins"] or min(want["margins"]) >= 1e-7, want["margins"]      # (the condition, for this case)
    _compare(res, want, 1, k=k, label=f"{name} cached x, problem {k}")


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_moments(5, 1, x=xs, prior=(mu, tau))       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)          # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_moments(5, 1)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_moments(0, 1, x=xs)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_moments(5, 1, stride=bad, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_moments(5, 1, stride=bad, x=xs)
    assert ctx.particle_moments(5, 1, stride=2 ** 31 - 1, x=xs)["moments"].shape == (3, 1, 2, 12)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_moments(5, 1, ess_fraction=bad, x=xs)
    # more workgroups per problem than a launch holds: refused before any work, and the context stays usable
    with pytest.raises(NotImplementedError, match="particles per problem"):
        ctx.particle_moments(65535 * 64 + 1, 1, x=xs)
    # through the C ABI itself: a null moments, logw or state; lineage_ess, ess and resampled are optional
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    mom = np.empty((3, ctx.Np, 2, 12))
    call = lambda a, b, c: ctx._lib.vgpa_particle_moments(ctx._h, xx.ctypes.data, None, 5, 1, 1, 0.5, None, None, a, b, c, None, None, None)      # noqa: E731
    assert call(lw.ctypes.data, st.ctypes.data, None) == -1
    assert call(None, st.ctypes.data, mom.ctypes.data) == -1 and call(lw.ctypes.data, None, mom.ctypes.data) == -1
    assert call(lw.ctypes.data, st.ctypes.data, mom.ctypes.data) == 0
    assert np.array_equal(mom, ctx.particle_moments(5, 1, x=xs)["moments"])
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
        ode.particle_moments(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_moments(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_moments(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records_of_vargp_and_problem_batch():
    """ProblemBatch.particle_moments and VarGP.particle_moments: one SmoothingMoments per member, equal to the bare context's rows and to
    the restatement of index p; the 1-D models drop the last axis"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.particle_moments(17, SEED_BATCH, stride=2, x=x)
    d = 12
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(3, d, d))
    bare = pb._context().particle_moments(17, SEED_BATCH, stride=2, x=pb._stack(x), prior=prior)
    pb.close()
    assert len(recs) == 3
    for k, p in enumerate(ps):
        want = particle_moments_numpy(_fields(p["vgp"]), x[k], None, 17, SEED_BATCH, 0.5, index=k)
        assert not want["margins"] or min(want["margins"]) >= 1e-7, (k, want["margins"])      # (the condition, for these cases)
        rec = recs[k]
        assert isinstance(rec, va.SmoothingMoments) and len(rec) == 17 and rec.stride == 2
        assert np.array_equal(rec.moments, bare["moments"][k]) and np.array_equal(rec.log_w, bare["log_w"][k])
        assert np.array_equal(rec.mean, bare["moments"][k, :, 0]) and np.array_equal(rec.second, bare["moments"][k, :, 1])
        assert np.array_equal(rec.var, rec.second - rec.mean ** 2) and np.array_equal(rec.grid, np.arange(0, int(want["m1"].shape[0]), 2))
        assert np.array_equal(rec.lineage_ess, bare["lineage_ess"][k, :rec.obs_t.size + 1]) and np.array_equal(rec.obs_t, want["obs_t"])
        assert rec.lineage_ess_on_grid().shape == rec.grid.shape and np.isfinite(rec.log_evidence())
        _compare(bare, want, 2, k=k, label=f"ProblemBatch member {k}")
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.particle_moments(33, 3, x=v.initialization())
    v.invalidate()
    assert rec.mean.shape == rec.var.shape == rec.std.shape == (v.dim_n,) and rec.lineage_ess.size == rec.obs_t.size + 1
    assert np.all(rec.std >= 0.0) and rec.lineage_ess_on_grid()[-1] == rec.lineage_ess[np.searchsorted(rec.obs_t, v.dim_n - 1)]


def test_report_worst_deviations():
    """No check of its own: prints the largest deviations the comparisons of this module have seen in this process so far (run behind
    them, the figures DESIGN.md s.4.12 quotes); every comparison asserts its own bound in _compare."""
    print("worst deviations over the module, in units of their scales:", WORST)
