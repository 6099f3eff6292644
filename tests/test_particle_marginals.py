"""
The smoothing marginals on the grid under the particle filter's genealogy on the GPU (vgpa_particle_marginals).

Every comparison starts from data the device returned, and none has a tolerance but the one on q:
  * log_w, state, ess, resampled are particle_filter's and lineage_ess is particle_moments', array_equal;
  * mass is array_equal to the integer histogram, weighted by the returned q_final, of the device's own lineage paths --
    particle_paths(n_draw=n, slots=arange(n), stride=1) of the same context, seed and arguments, which are the filter's lineages to the
    bit (their end points are asserted equal to `state`); with ess_fraction = 0 of the paths sample_paths_weighted stores.  Both sides bin
    the same state bits with the same compares: there is no margin condition;
  * |q_final 2^-62 - W| <= 2^-62 + 1e-12 W with W normalised on the host from the returned log_w (1e-12: the bound test_particle_events.py
    holds the device's normalised weights to);
  * sum_b mass = sum_i q_final at every kept grid index and component; a second call gives the same bits.
The cases are those of tests/test_particle_events.py (the cases of tests/test_particle_filter.py that test_particle_filter_cpu.py clears), at
strides 1, 4 and Np + 3 with 1, 7 and 63 levels; the ladders are test_particle_marginals_cpu.reference's (the 10 % ... 90 % quantiles of the
restatement's visited values; the single level moved between two survivors where the median does not split them), which that file
holds to split the surviving lineages of every case into at least two bins somewhere.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights_cpu import TAGS
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import FRACTIONS, PLACEMENTS, QUIET, SEED, SEED_BATCH, batch_case, case, placement_case
from test_particle_marginals_cpu import LEVEL_COUNTS, ladder_of, mass_of_paths, reference

pytestmark = pytest.mark.gpu

WALK = ("log_w", "state", "ess", "resampled")
WORST = {"q": 0.0}      # the largest |q 2^-62 - W| / (2^-62 + 1e-12 W) the module has seen, printed by the last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _own_paths(ctx, n, seed, **kw):
    """(B, n, Np, D): the lineage path of every final slot from the device itself, and the run's dict"""
    run = ctx.particle_paths(n, seed, n, stride=1, slots=np.arange(n), **kw)
    return run["paths"], run


def _check_q(got, k, label=""):
    lw = got["log_w"][k]
    w = np.exp(lw - np.max(lw))
    w = w / np.sum(w)
    q = got["q_final"][k]
    assert q.dtype == np.uint64 and int(q.astype(object).sum()) < 2 ** 63, label
    ratio = float(np.max(np.abs(q.astype(float) * 2.0 ** -62 - w) / (2.0 ** -62 + 1e-12 * w)))
    WORST["q"] = max(WORST["q"], ratio)
    assert ratio <= 1.0, (label, ratio)


def _check_mass(got, k, paths, ladder, stride, label=""):
    """problem k's mass against the integer histogram of the lineage paths (n, Np, D) weighted by the returned q_final"""
    mass, q = got["mass"][k], got["q_final"][k]
    n_keep = (paths.shape[1] - 1) // stride + 1
    assert mass.dtype == np.uint64 and mass.shape == (n_keep, paths.shape[2], ladder.shape[1] + 1), (label, mass.shape)
    assert np.array_equal(mass, mass_of_paths(paths, q, ladder, stride)), label
    assert np.all(mass.sum(axis=2, dtype=np.uint64) == q.sum(dtype=np.uint64)), label
    _check_q(got, k, label)


def _check(ctx, n, seed, ladders, strides, k=0, label="", **kw):
    """every (stride, ladder) of one run: the walk is the filter's, lineage_ess the moments', mass the histogram of the device's own paths.
    Returns the dicts by (stride, levels)."""
    flt = ctx.particle_filter(n, seed, **kw)
    mom = ctx.particle_moments(n, seed, stride=1, **kw)
    paths, run = _own_paths(ctx, n, seed, **kw)
    assert np.array_equal(run["log_w"], flt["log_w"]) and np.array_equal(paths[:, :, -1], flt["state"]), label
    out = {}
    for stride in strides:
        for ladder in ladders:
            count = ladder.shape[-1]
            got = out[(stride, count)] = ctx.particle_marginals(n, seed, ladder, stride=stride, **kw)
            for key in WALK:
                assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (label, stride, count, key)
            assert np.array_equal(got["lineage_ess"], mom["lineage_ess"]), (label, stride, count)
            lad = ladder if ladder.ndim == 2 else ladder[k]
            _check_mass(got, k, paths[k], lad, stride, f"{label} stride={stride} L={count}")
    return out


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_mass_exact(contexts, tag, start, n_paths, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 4, 5, 64 (k_sample_small<1, 3, 4>, k_sample_mfma<16, 32, 48, 64>; 17 odd; 64 without a padding row); one lane, a
    partial 16-path tile inside a partial block, a second workgroup, a second 256-slot workgroup at D <= 4 and a second pass of the integer
    descendant sums; collapsed clouds (most Q are 0) and the quiet cases' mix of gathered and carried clouds; every grid index, every
    fourth and index 0 alone; 1, 7 and 63 levels"""
    q, x, x0 = case(tag)
    ref = reference(("grid", tag, start, n_paths, ess_fraction))
    kw = dict(ess_fraction=ess_fraction, x=x, x0=x0 if start == "given" else None, prior=_prior(q))
    ctx = _ctx(contexts, tag)
    label = f"{tag} n={n_paths} {start} f={ess_fraction}"
    runs = _check(ctx, n_paths, SEED, [ref["ladders"][c] for c in LEVEL_COUNTS], (1, 4, int(q.n_pts) + 3), label=label, **kw)
    first = runs[(1, 7)]
    assert np.array_equal(first["resampled"][0, :ref["ess"].size], ref["resampled"]), label
    assert np.array_equal(runs[(4, 7)]["mass"], first["mass"][:, ::4]) and np.array_equal(runs[(4, 63)]["q_final"], first["q_final"])
    again = ctx.particle_marginals(n_paths, SEED, ref["ladders"][7], stride=1, **kw)
    for key in first:
        assert np.array_equal(again[key], first[key]), (label, key)
    if n_paths > 1 and np.count_nonzero(first["q_final"]) > 1:      # (the condition the CPU file asserts on the restatement, seen on the device)
        for count in LEVEL_COUNTS:
            assert np.count_nonzero(runs[(1, count)]["mass"][0], axis=2).max() >= 2, (label, count)


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_devices_stored_paths(contexts, tag, start):
    """ess_fraction = 0: the mass is the histogram of the paths sample_paths_weighted stores for the same seed; every row of Q is q"""
    q, x, x0 = case(tag)
    ref = reference(("grid", tag, start, 17, 0.0))
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=s0)[0][0]
    for stride, count in ((1, 63), (4, 7), (int(q.n_pts) + 3, 1)):
        got = ctx.particle_marginals(17, SEED, ref["ladders"][count], stride=stride, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q))
        assert not got["resampled"].any()
        _check_mass(got, 0, paths, ref["ladders"][count], stride, f"{tag} {start} f=0 stride={stride} L={count}")


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p", "l96d64"])
def test_every_particle_starts_on_a_level(contexts, tag):
    """x0 given = c_l: c_l < x is false, so at grid index 0 the whole mass lies in bin l of every component"""
    q, x, x0 = case(tag)
    d = int(q.dim_d)
    x0 = np.reshape(np.asarray(x0, dtype=float), d)
    ctx = _ctx(contexts, tag)
    kw = dict(ess_fraction=0.5, x=x, x0=x0, prior=_prior(q))
    for l in (0, 1, 2):
        ladder = x0[:, None] + (np.arange(3) - l)[None, :] * 0.25
        ladder[:, l] = x0
        got = _check(ctx, 17, SEED, [ladder], (1,), label=f"{tag} level {l} = x0", **kw)[(1, 3)]
        total = got["q_final"][0].sum(dtype=np.uint64)
        assert np.all(got["mass"][0, 0, :, l] == total) and np.all(np.delete(got["mass"][0, 0], l, axis=1) == 0), (tag, l)


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (index 0 counted with stretch 0's weights in an empty first segment), adjacent indices (segments of one
    step), Np - 1 (an empty last stretch)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for given in (False, True):
        ref = reference(("placement", model, d, obs_at, given))
        kw = dict(ess_fraction=1.0, x=x, x0=np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1 if given else None, prior=_prior(q))
        label = f"{model} {obs_at} {'given' if given else 'drawn'}"
        runs = _check(ctx, 17, SEED, [ref["ladders"][7], ref["ladders"][63]], (1, 4), label=label, **kw)
        assert np.array_equal(runs[(1, 7)]["resampled"][0], ref["resampled"]), label
    ctx.close()


def test_no_observations():
    """a context without observations: one segment, one stretch, the final weights"""
    q, x = placement_case("L96", 12, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, 12)))
    ctx = va.Context("L96", "euler", 12, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), 12) + 0.1
    kw = dict(ess_fraction=0.5, x=x, x0=x0)
    paths, _ = _own_paths(ctx, 17, SEED, **kw)
    ladder = ladder_of(paths[0], 7)
    got = _check(ctx, 17, SEED, [ladder], (1, 3), label="no observations", **kw)[(1, 7)]
    assert got["ess"].shape == (1, 0) and got["lineage_ess"].shape == (1, 1)
    ctx.close()


@pytest.mark.parametrize("model,d,n_pts", [("OU", 1, 2100), ("L96", 5, 2100)])
def test_a_long_grid(model, d, n_pts):
    """about 2100 grid indices, five segments: many times more kept indices than a workgroup has lanes, every one its own rows of mass"""
    q, x = make_problem(model, d, n_pts, method="euler", obs_at=[0, 700, 1400, 1401, n_pts - 1])
    ctx = gpu_context(q)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    kw = dict(ess_fraction=0.5, x=x, x0=x0, prior=_prior(q))
    paths, _ = _own_paths(ctx, 65, SEED, **kw)
    runs = _check(ctx, 65, SEED, [ladder_of(paths[0], 31)], (1, 7), label=f"{model} Np={n_pts}", **kw)
    assert runs[(1, 31)]["mass"].shape == (1, n_pts, d, 32) and np.count_nonzero(runs[(1, 31)]["mass"][0], axis=2).max() >= 2
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows_and_ladders(model, d):
    """B = 3 with own observation times and counts, theta, Sigma, R, H and ladders: every problem's mass is the histogram of its own paths
    on its own ladder; the last problem is bit for bit the same beside two other neighbours; problem 0 alone gives problem 0's rows"""
    runs = {}
    ladders = np.stack([reference(("batch", model, d, 20, k))["ladders"][7] for k in range(3)])
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        kw = dict(ess_fraction=0.5, x=xs, prior=prior)
        for k in range(3):
            got = _check(ctx, 40, SEED_BATCH, [ladders], (3,), k=k, label=f"{model} batch {first} problem {k}", **kw)[(3, 7)]
        runs[first] = first_problem = got
        ctx.close()
        if first == 20:
            q = probs[0]
            one = va.Context(model, "euler", d, 41, q.dt, sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0, obs_t=q.obs_t, obs_y=q.obs_y,
                             obs_noise=q.obs_noise, obs_h=q.obs_h)
            # (the same counters: its states are problem 0's of the batch, its mass the histogram of its own paths under its own q_final)
            alone = _check(one, 40, SEED_BATCH, [ladders[0]], (3,), label=f"{model} problem 0 alone", ess_fraction=0.5, x=xs[0],
                           prior=(prior[0][:1], prior[1][:1]))[(3, 7)]
            one.close()
            assert np.array_equal(alone["state"][0], first_problem["state"][0])
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["mass"][0], runs[50]["mass"][0])
    # another problem's ladder changes the problem's mass
    probs, xs = batch_case(model, d, 20)
    ctx = _batch_context(model, d, probs)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
    swapped = ctx.particle_marginals(40, SEED_BATCH, ladders[[1, 2, 0]], stride=3, ess_fraction=0.5, x=xs, prior=prior)
    ctx.close()
    assert all(not np.array_equal(swapped["mass"][k], runs[20]["mass"][k]) for k in range(3)) and np.array_equal(swapped["q_final"], runs[20]["q_final"])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_marginals(x=None) are bit for bit what
    they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
    dim = int(probs[0].dim_d)
    ladders = np.stack([np.reshape(np.asarray(q.m0, dtype=float), dim)[:, None] + np.linspace(-1.0, 1.0, 5)[None, :] for q in probs])

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_marginals(9, 4, ladders, stride=2, prior=prior) for step in order]
        if order[0] == "marginals":      # the cached x is the x: the same bits as with it given
            given = ctx.particle_marginals(9, 4, ladders, stride=2, x=xs, prior=prior)
            assert all(np.array_equal(given[key], out[0][key]) for key in given)
        ctx.close()
        return out

    a1, res, a2 = run(["record", "marginals", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["marginals", "record"])
    for key in res:
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    assert np.all(res["mass"].sum(axis=3, dtype=np.uint64) == res["q_final"].sum(axis=1, dtype=np.uint64)[:, None, None])


def test_records_of_vargp_and_problem_batch():
    """VarGP.particle_marginals and ProblemBatch.particle_marginals: one SmoothingMarginals per member, equal to the bare context's rows; the
    default ladder is gaussian_ladder of the posterior at x; the 1-D models drop the component axis"""
    from vgpa_amd.particles import gaussian_ladder
    v = build_problem("DW", "euler", 0.5)["vgp"]
    x = v.initialization()
    rec = v.particle_marginals(300, 11, x=x)
    assert isinstance(rec, va.SmoothingMarginals) and len(rec) == 300 and rec.mass.shape == (v.dim_n, 1, 32) and rec.levels.shape == (1, 31)
    out = v.arg_out
    assert np.array_equal(rec.levels, gaussian_ladder(out["mt"], out["st"]))
    bare = v._context().particle_marginals(300, 11, rec.levels, x=np.asarray(x, dtype=float), prior=v._prior())
    assert np.array_equal(rec.mass, bare["mass"][0]) and np.array_equal(rec.q_final, bare["q_final"][0]) and np.array_equal(rec.log_w, bare["log_w"][0])
    assert np.array_equal(rec.lineage_ess, bare["lineage_ess"][0, :rec.obs_t.size + 1])
    flt = v.particle_filter(300, 11, x=x)
    assert np.array_equal(rec.log_w, flt.log_w) and rec.log_evidence() == flt.log_evidence()
    cdf, lo, hi = rec.cdf(), *rec.band(0.05, 0.95)
    assert cdf.shape == (v.dim_n, 31) and np.all(np.diff(cdf, axis=1) >= 0.0) and cdf.min() >= 0.0 and cdf.max() <= 1.0
    assert lo.shape == hi.shape == (v.dim_n,) and np.all(lo <= hi) and np.all(rec.total() == rec.q_final.sum(dtype=np.uint64))
    assert np.allclose(rec.hist().sum(axis=1), 1.0, rtol=1e-15, atol=0.0) and np.array_equal(rec.exceedance(15), 1.0 - cdf[:, 15])
    print("double well: 5 % / 95 % quantiles at the last grid index", lo[-1], hi[-1], " modes there", rec.modes(v.dim_n - 1),
          " P(x > level 15 =", rec.levels[0, 15], ") along the window", np.round(rec.exceedance(15)[::20], 3))
    coarse = v.particle_marginals(300, 11, rec.levels[0], stride=7, x=x)
    assert np.array_equal(coarse.mass, rec.mass[::7]) and np.array_equal(coarse.q_final, rec.q_final)
    pb = va.ProblemBatch([v])
    recs = pb.particle_marginals(300, 11, x=x)
    pb.close()
    assert len(recs) == 1 and isinstance(recs[0], va.SmoothingMarginals)
    assert np.array_equal(recs[0].levels, rec.levels) and np.array_equal(recs[0].mass, rec.mass) and np.array_equal(recs[0].q_final, rec.q_final)
    assert np.array_equal(recs[0].ess, rec.ess) and np.array_equal(recs[0].resampled, rec.resampled)
    v.invalidate()
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(2)]
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    xb = pb.initialization()
    ladders = np.stack([np.linspace(-8.0, 12.0, 9) + 0.1 * k for k in range(2)])[:, None, :].repeat(12, axis=1)
    recs = pb.particle_marginals(17, SEED_BATCH, ladders, stride=2, x=xb)
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(2, 12, 12))
    bare = pb._context().particle_marginals(17, SEED_BATCH, ladders, stride=2, x=pb._stack(xb), prior=prior)
    pb.close()
    for k, rec in enumerate(recs):
        assert rec.stride == 2 and np.array_equal(rec.levels, ladders[k]) and np.array_equal(rec.mass, bare["mass"][k])
        assert np.array_equal(rec.q_final, bare["q_final"][k]) and np.array_equal(rec.lineage_ess, bare["lineage_ess"][k, :rec.obs_t.size + 1])
        assert rec.cdf().shape == (rec.grid.size, 12, 9) and rec.modes(0).shape == (12,)


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    ladders = np.tile(np.linspace(-4.0, 10.0, 7), (3, 12, 1))
    usable = lambda: ctx.particle_marginals(5, 1, ladders, x=xs, prior=(mu, tau))       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)                      # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_marginals(5, 1, ladders)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_marginals(0, 1, ladders, x=xs)
    for bad in (2 ** 31, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_marginals(bad, 1, ladders, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_marginals(5, 1, ladders, stride=bad, x=xs)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_marginals(5, 1, ladders, stride=bad, x=xs)
    assert ctx.particle_marginals(5, 1, ladders, stride=2 ** 31 - 1, x=xs)["mass"].shape == (3, 1, 12, 8)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_marginals(5, 1, ladders, ess_fraction=bad, x=xs)
    # more workgroups per problem than a launch holds: refused before any work, and the context stays usable
    with pytest.raises(NotImplementedError, match="particles per problem"):
        ctx.particle_marginals(65535 * 64 + 1, 1, ladders, x=xs)
    assert same(usable(), ref)
    # through the C ABI itself: null arguments, the number of levels, the ladders
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    mass, qf = np.empty((3, ctx.Np, 12, 8), dtype=np.uint64), np.empty((3, 5), dtype=np.uint64)

    def call(lev=ladders, count=7, a=lw, b=st, c=mass, stride=1):
        lev = None if lev is None else np.ascontiguousarray(lev, dtype=float)
        ptr = lambda v: None if v is None else v.ctypes.data      # noqa: E731
        return ctx._lib.vgpa_particle_marginals(ctx._h, xx.ctypes.data, None, 5, stride, 1, 0.5, None, None, ptr(lev), count, ptr(a), ptr(b), ptr(c),
                                                qf.ctypes.data, None, None, None)

    err = lambda: ctx._lib.vgpa_last_error(ctx._h)      # noqa: E731
    assert call(lev=None) == -1 and call(c=None) == -1 and call(a=None) == -1 and call(b=None) == -1
    for bad in (0, 64, -1):
        assert call(count=bad) == -1 and b"n_levels" in err()
    assert call(stride=0) == -1 and b"stride" in err()
    for bad in (np.nan, np.inf, -np.inf):
        lev = ladders.copy()
        lev[2, 11, 3] = bad
        assert call(lev=lev) == -1 and b"finite (problem 2, component 11" in err()
    for at, val in ((3, ladders[0, 0, 2]), (6, ladders[0, 0, 0])):      # (equal neighbours; a level below its predecessor)
        lev = ladders.copy()
        lev[1, 4, at] = val
        assert call(lev=lev) == -1 and b"strictly increasing (problem 1, component 4" in err()
    assert call() == 0
    bare = ctx.particle_marginals(5, 1, ladders, x=xs)      # (no prior, as the calls above)
    assert np.array_equal(mass, bare["mass"]) and np.array_equal(qf, bare["q_final"])
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
        ode.particle_marginals(2, 1, [0.0, 1.0], x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_marginals(2, 1, [0.0, 1.0], x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_marginals(2, 1, [0.0, 8.0], x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_report_worst_deviations():
    """No check of its own: prints the largest |q 2^-62 - W| in units of its bound that the comparisons of this module have seen in this
    process so far (the figure DESIGN.md s.4.21 quotes); every comparison asserts its own bound in _check_q."""
    print("worst |q_final 2^-62 - W| / (2^-62 + 1e-12 W) over the module:", WORST)
