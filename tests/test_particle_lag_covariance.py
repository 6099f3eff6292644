"""
The two-time moments of the particle smoother on the GPU (vgpa_particle_lag_covariance, vgpa_path_cross_moments).

The restatement, the floor, the runs and the anchors are test_particle_lag_covariance_cpu.py's, which asserts without a device that the
floor covers the oracle on every run of this module.  What is compared here:
  1. exact operands through path_cross_moments: integer-valued paths, |x| <= 2^10, no symmetry in (a, b) or between the two times,
     integer weights 1 .. 8 (and NULL weights with n = 64): array_equal to the int64 einsum, for every kernel instantiation;
  2. the fused entry against the longdouble contraction of the trajectories the device itself returns (particle_paths(n_draw = n,
     slots = arange(n))) with its own log_w: e_k <= 32 max(e_o, 1) in units of the floor, no entry excluded;
  3. bit for bit: the walk against particle_filter, lineage_ess against particle_moments, a second call, the batch around a problem, the
     other anchors of a call, a kept row at stride 4 against stride 1, and with one particle the fp64 product itself;
  4. at an anchor's own index, cross against particle_covariance's second: two evaluations of one sum, held to 32 2^-53 times the sum of
     this module's size and extended_ref.weighted_sum's;
  5. ess_fraction = 0 against path_cross_moments on sample_paths_weighted's paths; 6. the cached state; 7. the errors.
Every grid has at most 41 points; the contexts are those of tests/test_particle_filter.py.
"""
import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import PLACEMENTS, SEED, SEED_BATCH, batch_case, case, placement_case
from test_particle_lag_covariance_cpu import F64, LD, RUNS, SIZES, anchors_of, compare, lag_cross_numpy
from test_particle_rounding_cpu import FACTOR, UNIT
from test_path_weights_cpu import TAGS

pytestmark = pytest.mark.gpu

WALK = ("log_w", "state", "ess", "resampled")
WORST = {}
DIMS = (1, 3, 4, 5, 12, 17, 40, 64)      # the lane kernel (1, 3, 4), NT = 16 (5, 12), 32 (17), 48 (40), 64 (64 = NT: no padding row)


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _family(d):
    return "k_path_cross_lane" if d <= 4 else f"k_path_cross_mfma<{16 * ((d + 15) // 16)}>"


def _operator(cache, d):
    """an ODE-only context without a model, batch 2: all path_cross_moments needs"""
    if ("operator", d) not in cache:
        cache[("operator", d)] = va.Context("NONE", "euler", d, 10, 0.01, sigma=np.eye(d), batch=2)
    return cache[("operator", d)]


def _call(ctx, tag, start, n, frac, stride, anchors, method="particle_lag_covariance", **more):
    q, x, x0 = case(tag)
    args = (anchors,) if method == "particle_lag_covariance" else ()
    return getattr(ctx, method)(n, SEED, *args, stride=stride, ess_fraction=frac, x=x, x0=x0 if start == "given" else None, prior=_prior(q), **more)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
def integer_paths(b, n, n_keep, d):
    p, i, k, a = np.meshgrid(np.arange(b), np.arange(n), np.arange(n_keep), np.arange(d), indexing="ij")
    return ((p * 15485863 + i * 7919 + k * 104729 + a * 1299709) % 2047 - 1023).astype(np.int64)


@pytest.mark.parametrize("n", SIZES + (64,))
@pytest.mark.parametrize("d", DIMS)
def test_exact_operands(contexts, d, n):
    """rows >= D and paths >= n contribute zeros, every weight meets its own path, a and b and the two times keep their sides: the sums
    are integers below 2^53 and every product and partial sum is exact.  n = 64: NULL weights, 1 / 64 each."""
    ctx = _operator(contexts, d)
    n_keep, rows = 7, np.array([5, 0, 6, 5])
    x = integer_paths(2, n, n_keep, d)
    assert np.abs(x).max() <= 2 ** 10 and (d == 1 or not np.array_equal(x, x[..., ::-1])) and not np.array_equal(x[:, :, rows[0]], x[:, :, rows[1]])
    w = None if n == 64 else 1 + (np.arange(2 * n).reshape(2, n) * 5 + 3) % 8
    wi = np.ones((2, n), dtype=np.int64) if w is None else w
    mean, cross = ctx.path_cross_moments(x.astype(F64), rows, weights=None if w is None else w.astype(F64))
    want_m, want_c = np.einsum("pi,pika->pka", wi, x), np.einsum("pi,pika,piqb->pqkab", wi, x, x[:, :, rows])
    scale = 64 if w is None else 1
    assert np.abs(want_c).max() < 2 ** 53 and mean.shape == (2, n_keep, d) and cross.shape == (2, 4, n_keep, d, d)
    assert np.array_equal(mean * scale, want_m) and np.array_equal(cross * scale, want_c)
    assert np.array_equal(cross[:, 0], cross[:, 3])      # a row asked for twice


# ---- 2, 3 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=lambda r: "-".join(map(str, r)))
def test_against_the_devices_own_trajectories(contexts, run):
    """mean and cross against the longdouble contraction of the trajectories particle_paths returns for every final slot, with the log_w of
    the same call; the walk is the filter's, lineage_ess the moments', a second call gives the same bits"""
    tag, start, n, frac, stride = run
    q = case(tag)[0]
    ctx = _ctx(contexts, tag)
    anchors = anchors_of(int(q.n_pts), stride, q.obs_t)
    got = _call(ctx, tag, start, n, frac, stride, anchors)
    pth = _call(ctx, tag, start, n, frac, stride, None, "particle_paths", n_draw=n, slots=np.arange(n))
    flt = ctx.particle_filter(n, SEED, ess_fraction=frac, x=case(tag)[1], x0=case(tag)[2] if start == "given" else None, prior=_prior(q))
    mom = _call(ctx, tag, start, n, frac, stride, None, "particle_moments")
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]) and np.array_equal(pth[key], flt[key]), key
    assert np.array_equal(got["lineage_ess"], mom["lineage_ess"])
    d = int(q.dim_d)
    assert got["mean"].shape == (1, pth["paths"].shape[2], d) and got["cross"].shape == (1, anchors.size, pth["paths"].shape[2], d, d)
    fails = compare(WORST, "-".join(map(str, run)), _family(d), got["mean"][0], got["cross"][0], pth["paths"][0], anchors // stride, log_w=got["log_w"][0])
    assert not fails, fails
    again = _call(ctx, tag, start, n, frac, stride, anchors)
    for key in got:
        assert np.array_equal(again[key], got[key]), key
    if n == 1:      # W = 1: fma(x(k)[a], 1 x(s)[b], 0) is the fp64 product
        x = pth["paths"][0, 0]
        assert np.array_equal(got["cross"][0], x[None, :, :, None] * x[anchors // stride][:, None, None, :]) and np.array_equal(got["mean"][0], x)


@pytest.mark.parametrize("tag", TAGS)
def test_anchors_and_strides_do_not_matter(contexts, tag):
    """an anchor's block does not depend on the other anchors of the call ({0}, {the last kept index}, three anchors), and a kept row at
    stride 4 is the row of the same grid index at stride 1"""
    q = case(tag)[0]
    ctx = _ctx(contexts, tag)
    n_pts = int(q.n_pts)
    three = anchors_of(n_pts, 4, q.obs_t)      # (kept at both strides)
    one = _call(ctx, tag, "drawn", 17, 0.5, 1, three)
    four = _call(ctx, tag, "drawn", 17, 0.5, 4, three)
    assert np.array_equal(four["mean"], one["mean"][:, ::4]) and np.array_equal(four["cross"], one["cross"][:, :, ::4])
    assert np.array_equal(four["lineage_ess"], one["lineage_ess"])
    for s in (three[0], three[-1]):
        alone = _call(ctx, tag, "drawn", 17, 0.5, 4, [s])
        assert np.array_equal(alone["cross"][:, 0], four["cross"][:, list(three).index(s)]) and np.array_equal(alone["mean"], four["mean"])
    last = _call(ctx, tag, "drawn", 17, 0.5, 1, [n_pts - 1])      # the last grid index itself
    assert np.array_equal(last["mean"], one["mean"])
    if (n_pts - 1) % 4 == 0:
        assert np.array_equal(last["cross"][:, 0], one["cross"][:, -1])


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with ragged observation counts: every problem against the contraction of its own returned trajectories, and the last problem's
    block bit for bit the same beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        anchors = np.array([0, 13, 40])      # (13: an observation of the first problem alone)
        runs[first] = got = ctx.particle_lag_covariance(40, SEED_BATCH, anchors, ess_fraction=0.5, x=xs, prior=prior)
        pth = ctx.particle_paths(40, SEED_BATCH, 40, ess_fraction=0.5, x=xs, prior=prior, slots=np.arange(40))
        flt = ctx.particle_filter(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        mom = ctx.particle_moments(40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        ctx.close()
        for key in WALK:
            assert np.array_equal(got[key], flt[key]), key
        assert np.array_equal(got["lineage_ess"], mom["lineage_ess"])
        for k in range(3):
            fails = compare(WORST, f"{model} batch {first} problem {k}", _family(d), got["mean"][k], got["cross"][k], pth["paths"][k], anchors, log_w=got["log_w"][k])
            assert not fails, fails
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["cross"][0], runs[50]["cross"][0])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_own_index_against_particle_covariance(contexts, tag):
    """cross[q][s / stride] and second[s / stride]: final weights on the lineages' repeated states against descendant weights on the
    distinct ones (the CPU module asserts that the two restatements agree within the plain sum of the two floors)"""
    q = case(tag)[0]
    ctx = _ctx(contexts, tag)
    anchors = anchors_of(int(q.n_pts), 1, q.obs_t)
    got = _call(ctx, tag, "given", 65, 0.5, 1, anchors)
    cov = _call(ctx, tag, "given", 65, 0.5, 1, None, "particle_covariance")
    pth = _call(ctx, tag, "given", 65, 0.5, 1, None, "particle_paths", n_draw=65, slots=np.arange(65))
    paths, lw = pth["paths"][0], got["log_w"][0]
    size = lag_cross_numpy(paths, None, anchors, LD, log_w=lw)[3]
    worst = 0.0
    for i, s in enumerate(anchors):
        size2 = xr.weighted_sum(lw, np.einsum("na,nb->nab", paths[:, s].astype(LD), paths[:, s].astype(LD)), LD)[1]
        diff = np.abs(got["cross"][0, i, s].astype(LD) - cov["second"][0, s].astype(LD))
        bound = UNIT * (size[i, s] + size2)
        worst = max(worst, float(np.max(np.where(diff == 0, LD(0), diff / np.where(bound > 0, bound, LD(1))))))
        assert np.all(diff <= FACTOR * bound), (tag, s, worst)
    assert np.array_equal(got["lineage_ess"], cov["lineage_ess"])
    print(tag, "cross at the anchor's own index against second, in units of 2^-53 (size + size):", worst)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_operator(contexts, tag, start):
    """ess_fraction = 0: the trajectories are sample_paths_weighted's paths, and the result is path_cross_moments on them with the
    normalised weights"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    anchors = anchors_of(int(q.n_pts), 1, q.obs_t)
    got = _call(ctx, tag, start, 17, 0.0, 1, anchors)
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=x0 if start == "given" else None)[0]
    lw = got["log_w"][0]
    assert not got["resampled"].any()
    d = int(q.dim_d)
    fails = compare(WORST, f"{tag} {start} f=0", _family(d), got["mean"][0], got["cross"][0], paths[0], anchors, log_w=lw)
    w = xr.normalised_weights(lw, F64)[0]
    mean, cross = ctx.path_cross_moments(paths, anchors, weights=w[None])
    fails += compare(WORST, f"{tag} {start} f=0, the operator", _family(d), mean[0], cross[0], paths[0], anchors, W=w)
    assert not fails, fails
    size = lag_cross_numpy(paths[0], None, anchors, LD, log_w=lw)[3]
    assert np.all(np.abs(cross[0].astype(LD) - got["cross"][0]) <= FACTOR * UNIT * size)      # ... and the two agree within the floor's bound


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_lag_covariance(x=None) and
    path_cross_moments are bit for bit what they are without the calls (the scheme of test_sample_paths.test_the_cache_is_not_touched):
        A: free_energy, record, the calls, record      B: free_energy, record, record      C: free_energy, the calls, record"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
    n_pts = int(probs[0].n_pts)
    anchors = sorted({0, (n_pts - 1) // 10 * 5, (n_pts - 1) // 5 * 5})
    given = np.random.default_rng(8).standard_normal((nb, 6, 3, int(probs[0].dim_d)))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def calls(ctx):
        res = ctx.particle_lag_covariance(9, 4, anchors, stride=5, prior=prior)
        res["given mean"], res["given cross"] = ctx.path_cross_moments(given, [2, 0])
        return res

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else calls(ctx) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "calls", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["calls", "record"])
    for key in res:
        assert np.array_equal(res[key], res_c[key]), key
    assert np.all(np.isfinite(res["cross"])) and np.all(np.isfinite(res["given cross"]))
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    n_pts = int(probs[0].n_pts)
    last = (n_pts - 1) // 4 * 4
    usable = lambda: ctx.particle_lag_covariance(5, 1, [0, last], stride=4, x=xs)       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)                        # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_lag_covariance(5, 1, [0])
    ref = usable()
    assert ref["cross"].shape == (3, 2, last // 4 + 1, 12, 12)
    for bad, text in (([4, 0], "strictly increasing"), ([0, 0], "strictly increasing"), ([-4], "strictly increasing"), ([last + 4], "strictly increasing"),
                      ([0, 6], "no multiple of the stride"), ([], "null argument|at least 1")):
        with pytest.raises(ValueError, match=text):
            ctx.particle_lag_covariance(5, 1, bad, stride=4, x=xs)
    with pytest.raises(ValueError):
        ctx.particle_lag_covariance(0, 1, [0], x=xs)
    with pytest.raises(ValueError, match="stride"):
        ctx.particle_lag_covariance(5, 1, [0], stride=0, x=xs)
    with pytest.raises(ValueError, match="32 bits"):
        ctx.particle_lag_covariance(2 ** 31, 1, [0], x=xs)
    assert same(usable(), ref)
    # through the C ABI itself: null outputs and anchors
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    anc, mean, cross = np.array([0, last], dtype=np.int64), np.full((3, last // 4 + 1, 12), 3.0), np.full((3, 2, last // 4 + 1, 12, 12), 3.0)
    call = lambda n, a, m, c, lw=lw, st=st: ctx._lib.vgpa_particle_lag_covariance(      # noqa: E731
        ctx._h, xx.ctypes.data, None, 5, 4, 1, 0.5, None, None, n, a, None if lw is None else lw.ctypes.data, None if st is None else st.ctypes.data, m, c, None, None, None)
    assert call(2, None, mean.ctypes.data, cross.ctypes.data) == -1 and call(2, anc.ctypes.data, None, cross.ctypes.data) == -1
    assert call(2, anc.ctypes.data, mean.ctypes.data, None) == -1 and call(0, anc.ctypes.data, mean.ctypes.data, cross.ctypes.data) == -1
    assert call(2, anc.ctypes.data, mean.ctypes.data, cross.ctypes.data, lw=None) == -1 and call(2, anc.ctypes.data, mean.ctypes.data, cross.ctypes.data, st=None) == -1
    assert np.all(mean == 3.0) and np.all(cross == 3.0)
    assert call(2, anc.ctypes.data, mean.ctypes.data, cross.ctypes.data) == 0
    assert np.array_equal(mean, ref["mean"]) and np.array_equal(cross, ref["cross"])
    # the size refusals, before any work: more particles than the lineage walk takes (D = 12)
    cross[:] = 3.0
    rc = ctx._lib.vgpa_particle_lag_covariance(ctx._h, xx.ctypes.data, None, 2 ** 31 - 1, 4, 1, 0.5, None, None, 2, anc.ctypes.data, lw.ctypes.data, st.ctypes.data,
                                               mean.ctypes.data, cross.ctypes.data, None, None, None)
    assert rc == -5 and b"walks every particle's trajectory, at most" in ctx._lib.vgpa_last_error(ctx._h) and np.all(cross == 3.0)
    assert same(usable(), ref)
    # a dense Sigma in force
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert same(usable(), ref)
    # the operator on the same context: its own refusals, and the context stays usable
    paths = np.random.default_rng(2).standard_normal((3, 4, 3, 12))
    for rows in ([3], [-1]):
        with pytest.raises(ValueError, match="does not lie in"):
            ctx.path_cross_moments(paths, rows)
    with pytest.raises(ValueError, match="null argument|at least 1"):
        ctx.path_cross_moments(paths, [])
    with pytest.raises(NotImplementedError, match="at most 65535 anchors"):
        ctx.path_cross_moments(paths[:, :1, :1], np.zeros(65536, dtype=int))
    one = np.zeros(65535, dtype=np.int32)      # more entries of cross than one array may have: 3 x 65535 x 2^27 x 144
    rc = ctx._lib.vgpa_path_cross_moments(ctx._h, paths.ctypes.data, None, 1, 2 ** 27, 65535, one.ctypes.data, mean.ctypes.data, cross.ctypes.data)
    assert rc == -5 and b"2^39 - 256 entries of cross" in ctx._lib.vgpa_last_error(ctx._h)
    rc = ctx._lib.vgpa_path_cross_moments(ctx._h, paths.ctypes.data, None, 2 ** 31 - 1, 2 ** 10, 1, one.ctypes.data, mean.ctypes.data, cross.ctypes.data)
    assert rc == -5 and b"2^35 entries" in ctx._lib.vgpa_last_error(ctx._h)
    assert ctx._lib.vgpa_path_cross_moments(ctx._h, None, None, 4, 3, 1, one.ctypes.data, mean.ctypes.data, cross.ctypes.data) == -1
    assert ctx._lib.vgpa_path_cross_moments(ctx._h, paths.ctypes.data, None, 4, 3, 1, one.ctypes.data, None, cross.ctypes.data) == -1
    m, c = ctx.path_cross_moments(paths, [2, 0])
    assert np.allclose(c, np.einsum("pika,piqb->pqkab", paths, paths[:, :, [2, 0]]) / 4, rtol=1e-13, atol=1e-15) and np.allclose(m, paths.mean(axis=1), rtol=1e-13, atol=1e-15)
    assert same(usable(), ref)
    ctx.close()
    # more entries than the trajectories may have (at D <= 4 the walk's grid.x holds any int32 count): refused before any work
    q, x = placement_case("L63", 3, PLACEMENTS[0])
    small = gpu_context(q)
    xx, lw, st, m3, c3 = np.ascontiguousarray(x), np.empty((1, 5)), np.empty((1, 5, 3)), np.full((1, 41, 3), 3.0), np.full((1, 1, 41, 3, 3), 3.0)
    zero = np.zeros(1, dtype=np.int64)
    rc = small._lib.vgpa_particle_lag_covariance(small._h, xx.ctypes.data, None, 2 ** 31 - 1, 1, 1, 0.5, None, None, 1, zero.ctypes.data, lw.ctypes.data, st.ctypes.data,
                                                 m3.ctypes.data, c3.ctypes.data, None, None, None)
    assert rc == -5 and b"2^35 entries" in small._lib.vgpa_last_error(small._h) and b"use a larger stride" in small._lib.vgpa_last_error(small._h) and np.all(c3 == 3.0)
    assert small.particle_lag_covariance(5, 1, [0], x=x)["cross"].shape == (1, 1, 41, 3, 3)
    small.close()
    # no model: ValueError for the fused entry, and the operator works; ODE-only: RuntimeError, and the operator works
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_lag_covariance(2, 1, [0], x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    assert ode.path_cross_moments(np.ones((2, 4, 3, 3)), [1])[1].shape == (2, 1, 3, 3, 3)
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_lag_covariance(2, 1, [0], x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    assert np.all(bare.path_cross_moments(np.ones((2, 4, 3, 3)), [1])[1] == 1.0)
    bare.close()
    # D > 64
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_lag_covariance(2, 1, [0], x=x)
    with pytest.raises(NotImplementedError, match="D <= 64"):
        big.path_cross_moments(np.ones((1, 2, 2, 72)), [0])
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records():
    """VarGP.particle_kernel and ProblemBatch.particle_kernel: one SmoothingLagCovariance per member, against the member's own
    SmoothingCovariance at the anchors; SmoothingPaths.lag_covariance on backward-simulation draws; the 1-D shapes"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(2)]
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    n_pts = int(ps[0]["vgp"].dim_n)
    anchors = [0, (n_pts - 1) // 8 * 4, (n_pts - 1) // 4 * 4]
    recs = pb.particle_kernel(33, SEED_BATCH, anchors, stride=4, x=x)
    covs = pb.particle_covariance(33, SEED_BATCH, stride=4, x=x)
    pb.close()
    assert len(recs) == 2
    for rec, cov in zip(recs, covs):
        assert isinstance(rec, va.SmoothingLagCovariance) and len(rec) == 33 and np.array_equal(rec.anchors, anchors)
        assert np.array_equal(rec.log_w, cov.log_w) and np.array_equal(rec.lineage_ess, cov.lineage_ess) and np.array_equal(rec.grid, cov.grid)
        for s in anchors:
            assert np.allclose(rec.cov(s, s), cov.cov[s // 4], rtol=0, atol=1e-9 * np.abs(cov.second[s // 4]).max())
        m, c = rec.joint()
        assert m.shape == (36,) and c.shape == (36, 36) and np.array_equal(c, c.T)
        # (two anchors: the block of either, two evaluations of one sum with the weight on the other side)
        assert np.allclose(rec.cov(anchors[2], anchors[1]), rec.cov(anchors[1], anchors[2]).T, rtol=0, atol=1e-12 * np.abs(cov.second).max())
    v = build_problem("OU", "euler", 0.5)["vgp"]
    x = v.initialization()
    n_pts = int(v.dim_n)
    rec = v.particle_kernel(33, 3, [0, n_pts - 1], x=x)
    assert rec.mean.shape == (n_pts,) and rec.cross.shape == (2, n_pts) and np.ndim(rec.cov(n_pts - 1, 0)) == 0 and rec.autocorrelation(0).shape == (n_pts,)
    bwd = v.backward_paths(33, 3, 16, x=x)
    ctx = va.Context("NONE", "euler", 1, 10, 0.01, sigma=np.eye(1))
    lag = bwd.lag_covariance([0, n_pts - 1], ctx)
    ctx.close()
    v.invalidate()
    dev = bwd.paths - bwd.mean()[None]
    assert np.allclose(lag.cov(n_pts - 1, 0), np.mean(dev[:, -1] * dev[:, 0]), rtol=0, atol=1e-12 * (1 + np.abs(bwd.paths).max() ** 2))
    assert np.all(np.isnan(lag.lineage_ess))


def test_print_worst():
    for key, val in sorted(WORST.items()):
        print(key, f"worst e_k / max(e_o, 1) = {val:.3f}")
