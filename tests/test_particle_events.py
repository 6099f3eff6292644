"""
Path events of the particle filter's lineages on the GPU (vgpa_particle_events).

The rows are compared exactly, twice: with the events evaluated on the host on the device's own lineage paths -- particle_paths(n_draw=n,
slots=arange(n), stride=1) of the same context and seed, which are the filter's lineages to the bit (their end points are asserted equal to
`state`) -- and with test_particle_events_cpu.reference, whose levels keep every visited state at least 1e-7 max(1, |c|) away from its
level (asserted there for every case of this file), far above the 1e-12 by which device and numpy states differ: T and N, the integers the
margin decides, exactly.  X is a state minus a level, so against numpy it can only be as close as the states themselves are: it is held to
1e-9 max(1, max |x|), the bound test_particle_filter.py holds the device's states to against the same restatement (against the device's
own paths it is exact like T and N).  The walk itself -- log_w,
state, ess, resampled -- is compared bit for bit with particle_filter.  The two reductions are held against the host on the device's own
rows and log-weights: the mean to a relative 1e-12 (the bound test_particle_statistics.py holds k_pf_stats_mean to), the first-passage
distribution to an absolute 1e-12 against the longdouble restatement (its values lie in [0, 1]), non-decreasing exactly.
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
from test_particle_events_cpu import event_rows, events_of_paths, reductions_longdouble, reference, sides_for

pytestmark = pytest.mark.gpu

WALK = ("log_w", "state", "ess", "resampled")
TOL = 1e-9


def _against_numpy(rows, want, scale, label=""):
    """the device's rows against the restatement's: T and N exactly, X as close as the device's states are to numpy's"""
    assert rows.shape == want.shape and np.array_equal(rows[:, 1:], want[:, 1:]), label
    err = float(np.max(np.abs(rows[:, 0] - want[:, 0])) / max(1.0, scale))
    print(label, "T, N exact;  |X - X of the restatement| / max(1, max |x|) =", err)
    assert err <= TOL, (label, err)


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


def _check_reductions(got, k, n_pts, stride, label=""):
    """mean and cdf of problem k against the host's reductions of the device's own rows and log-weights"""
    rows, lw = got["rows"][k], got["log_w"][k]
    w = np.exp(lw - np.max(lw))
    host = np.tensordot(w, rows, axes=(0, 0)) / np.sum(w)
    mean = got["mean"][k]
    assert np.array_equal(mean[host == 0.0], host[host == 0.0]), label
    mean_err = float(np.max(np.abs(mean - host)[host != 0.0] / np.abs(host[host != 0.0]), initial=0.0))
    want = reductions_longdouble(lw, rows, n_pts, stride)[1]
    cdf = got["cdf"][k]
    assert cdf.shape == want.shape and np.all(np.isfinite(cdf)), (label, cdf.shape, want.shape)
    cdf_err = float(np.max(np.abs(cdf - want)))
    print(label, "device mean vs host mean of its rows: rel.err", mean_err, " cdf vs longdouble restatement: abs.err", cdf_err,
          " P(crossed)", np.round(cdf[-1][:4], 4))
    assert mean_err <= 1e-12, (label, mean_err)
    assert cdf_err <= 1e-12, (label, cdf_err)
    assert np.all(np.diff(cdf, axis=0) >= 0.0), label


def _check(ctx, got, n, seed, levels, side, k=0, label="", **kw):
    """problem k of particle_events' dict (per_particle=True, stride 1): the walk is the filter's, the rows are the events of the device's own
    lineage paths, the reductions are the host's"""
    flt = ctx.particle_filter(n, seed, **kw)
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (label, key)
    paths, run = _own_paths(ctx, n, seed, **kw)
    assert np.array_equal(paths[k][:, -1], got["state"][k]) and np.array_equal(run["log_w"], got["log_w"]), label
    rows = got["rows"][k]
    assert np.array_equal(rows, events_of_paths(paths[k], levels, side)), label
    assert np.array_equal(rows[:, 1:], np.round(rows[:, 1:])) and rows[:, 1].max() <= paths.shape[2], label      # (exact integers; the sentinel is Np)
    _check_reductions(got, k, paths.shape[2], 1, label)


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET])
def test_rows_exact(contexts, tag, start, n_paths, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 5, 64 (NT = 16, 32, 48, 64; 17 odd; 64 without a padding row); one lane, a partial 16-path tile inside a
    partial block, a second workgroup of one path, more than one 256-slot pass of the resampling and distribution kernels; collapsed clouds
    (every row copied from one survivor) and the quiet cases' mix of copied and carried rows"""
    q, x, x0 = case(tag)
    ref = reference(("grid", tag, start, n_paths, ess_fraction))
    kw = dict(ess_fraction=ess_fraction, x=x, x0=x0 if start == "given" else None, prior=_prior(q))
    ctx = _ctx(contexts, tag)
    got = ctx.particle_events(n_paths, SEED, ref["levels"], side=ref["side"], per_particle=True, **kw)
    label = f"{tag} n={n_paths} {start} f={ess_fraction}"
    _check(ctx, got, n_paths, SEED, ref["levels"], ref["side"], label=label, **kw)
    assert np.array_equal(got["resampled"][0, :ref["ess"].size], ref["resampled"]), label
    _against_numpy(got["rows"][0], ref["rows"], float(np.max(np.abs(ref["visited"]))), label)


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", TAGS)
def test_without_resampling_against_the_devices_stored_paths(contexts, tag, start):
    """ess_fraction = 0: the rows are the events of the paths sample_paths_weighted stores for the same seed"""
    q, x, x0 = case(tag)
    ref = reference(("grid", tag, start, 17, 0.0))
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    got = ctx.particle_events(17, SEED, ref["levels"], side=ref["side"], ess_fraction=0.0, x=x, x0=s0, prior=_prior(q), per_particle=True)
    paths = ctx.sample_paths_weighted(17, SEED, stride=1, x=x, x0=s0)[0][0]
    assert np.array_equal(got["rows"][0], events_of_paths(paths, ref["levels"], ref["side"])) and not got["resampled"].any()
    _against_numpy(got["rows"][0], ref["rows"], float(np.max(np.abs(ref["visited"]))), f"{tag} {start} f=0")
    _check_reductions(got, 0, int(q.n_pts), 1, f"{tag} {start} f=0")


@pytest.mark.parametrize("tag", TAGS + QUIET)
def test_strides_and_repeatability(contexts, tag):
    """the first-passage distribution on the kept grid: strides 1, 3 and one that does not divide Np - 1; two calls give the same bits; the
    rows and the mean do not depend on the stride; without the rows the results are the same"""
    q, x, x0 = case(tag)
    n_pts = int(q.n_pts)
    ref = reference(("grid", tag, "given", 65, 0.5))
    ctx = _ctx(contexts, tag)
    odd = next(s for s in range(4, n_pts) if (n_pts - 1) % s)
    first = None
    for stride in (1, 3, odd):
        call = lambda per: ctx.particle_events(65, SEED, ref["levels"], side=ref["side"], stride=stride, ess_fraction=0.5, x=x, x0=x0,      # noqa: E731
                                               prior=_prior(q), per_particle=per)
        got, again, alone = call(True), call(True), call(False)
        assert got["cdf"].shape == (1, (n_pts - 1) // stride + 1, int(q.dim_d))
        for key in got:
            assert np.array_equal(got[key], again[key]), (tag, stride, key)
            assert (alone[key] is None) if key == "rows" else np.array_equal(got[key], alone[key]), (tag, stride, key)
        _check_reductions(got, 0, n_pts, stride, f"{tag} stride={stride}")
        first = first or got
        assert np.array_equal(got["rows"], first["rows"]) and np.array_equal(got["mean"], first["mean"])
        assert np.max(np.abs(got["cdf"] - first["cdf"][:, ::stride])) <= 2e-12, (tag, stride)      # (other bins, another association: both within 1e-12)
    _against_numpy(first["rows"][0], ref["rows"], float(np.max(np.abs(ref["visited"]))), tag)


@pytest.mark.parametrize("model,d,n_pts", [("OU", 1, 4500), ("L96", 5, 2100)])
def test_a_grid_longer_than_one_tile_of_bins(model, d, n_pts):
    """more kept grid indices than k_pf_events_cdf holds in LDS at a time (2048): the tiles behind one another, the carry between them"""
    q, x = make_problem(model, d, n_pts, method="euler", obs_at=[0, 700, 2047, 2048, n_pts - 1])
    ctx = gpu_context(q)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    kw = dict(ess_fraction=0.0, x=x, x0=x0, prior=_prior(q))      # (no resampling: 65 lineages that share nothing, so that their first passages spread)
    side = sides_for(d)
    early = _own_paths(ctx, 65, SEED, **kw)[0][0][:, :2048]
    levels = np.median(np.where(side > 0, early.max(axis=1), early.min(axis=1)), axis=0)      # half of the lineages cross before index 2048
    for stride in (1, 2):
        got = ctx.particle_events(65, SEED, levels, side=side, stride=stride, per_particle=True, **kw)
        if stride == 1:
            _check(ctx, got, 65, SEED, levels, side, label=f"{model} Np={n_pts}", **kw)
            t = got["rows"][0][:, 1]
            assert t.min() < 2048 <= t[t < n_pts].max(), (t.min(), t.max())      # (first passages on both sides of the tile boundary)
        _check_reductions(got, 0, n_pts, stride, f"{model} Np={n_pts} stride={stride}")
    ctx.close()


@pytest.mark.parametrize("tag", ["l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p"])
def test_a_state_on_the_level_is_not_in_the_event(contexts, tag):
    """g = 0 exactly: every particle starts on the level of every component (a given start), and grid index 0 is not in the event"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    side = sides_for(int(q.dim_d))
    kw = dict(ess_fraction=0.5, x=x, x0=x0, prior=_prior(q))
    got = ctx.particle_events(17, SEED, x0, side=side, per_particle=True, **kw)
    assert np.all(got["rows"][0][:, 1] >= 1) and np.all(got["rows"][0][:, 0] >= 0.0) and np.all(got["cdf"][0, 0] == 0.0)
    _check(ctx, got, 17, SEED, x0, side, label=f"{tag} levels = x0", **kw)


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 with a resampling there (the rows of index 0 are gathered), adjacent indices, Np - 1"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for given in (False, True):
        ref = reference(("placement", model, d, obs_at, given))
        kw = dict(ess_fraction=1.0, x=x, x0=np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1 if given else None, prior=_prior(q))
        got = ctx.particle_events(17, SEED, ref["levels"], side=ref["side"], per_particle=True, **kw)
        label = f"{model} {obs_at} {'given' if given else 'drawn'}"
        _check(ctx, got, 17, SEED, ref["levels"], ref["side"], label=label, **kw)
        assert np.array_equal(got["resampled"][0], ref["resampled"]), label
        _against_numpy(got["rows"][0], ref["rows"], float(np.max(np.abs(ref["visited"]))), label)
        if obs_at[0] == 0 and not given:
            assert ref["resampled"][0] == 1      # (the condition: the start rows went through a gather; a given start has equal weights there)
    ctx.close()


def test_no_observations():
    """a context without observations: one segment, no resampling step"""
    q, x = placement_case("L96", 12, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, 12)))
    ctx = va.Context("L96", "euler", 12, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), 12) + 0.1
    levels, side = x0 + 0.05 * sides_for(12), sides_for(12)
    got = ctx.particle_events(17, SEED, levels, side=side, ess_fraction=0.5, x=x, x0=x0, per_particle=True)
    assert got["ess"].shape == (1, 0)
    _check(ctx, got, 17, SEED, levels, side, label="no observations", ess_fraction=0.5, x=x, x0=x0)
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows_levels_and_sides(model, d):
    """B = 3 with own observation times and counts, theta, Sigma, R, H, levels and sides: problem k is the single-problem restatement of
    index k; the last problem is bit for bit the same beside two other neighbours; the particles, rows and decisions of problem 0 are bit
    for bit those of a context that holds it alone (the same counters: problem index 0)"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        refs = [reference(("batch", model, d, first, k)) for k in range(3)]
        levels = np.stack([r["levels"] for r in refs])
        sides = np.stack([sides_for(d) * (-1 if k == 1 else 1) for k in range(3)])
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        kw = dict(ess_fraction=0.5, x=xs, prior=prior)
        runs[first] = got = ctx.particle_events(40, SEED_BATCH, levels, side=sides, stride=3, per_particle=True, **kw)
        flt = ctx.particle_filter(40, SEED_BATCH, **kw)
        paths, _ = _own_paths(ctx, 40, SEED_BATCH, **kw)
        ctx.close()
        for key in WALK:
            assert np.array_equal(got[key], flt[key]), key
        for k in range(3):
            label = f"{model} batch {first} problem {k}"
            assert np.array_equal(got["rows"][k], events_of_paths(paths[k], levels[k], sides[k])), label
            _against_numpy(got["rows"][k], event_rows(refs[k], levels[k], sides[k]), float(np.max(np.abs(refs[k]["visited"]))), label)
            assert np.array_equal(got["resampled"][k, :refs[k]["ess"].size], refs[k]["resampled"]), label
            _check_reductions(got, k, 41, 3, label)
        if first == 20:      # problem 0 alone: the same counters (problem index 0), the same bits
            q = probs[0]
            one = va.Context(model, "euler", d, 41, q.dt, sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0, obs_t=q.obs_t, obs_y=q.obs_y,
                             obs_noise=q.obs_noise, obs_h=q.obs_h)
            alone = one.particle_events(40, SEED_BATCH, levels[0], side=sides[0], stride=3, ess_fraction=0.5, x=xs[0], prior=(prior[0][:1], prior[1][:1]),
                                        per_particle=True)
            one.close()
            m = q.obs_t.size
            print(model, "problem 0 alone against problem 0 of the batch: max |log_w difference|", float(np.max(np.abs(alone["log_w"][0] - got["log_w"][0]))))
            for key in ("state", "rows", "resampled"):
                mine = got[key][0, :m] if key == "resampled" else got[key][0]
                assert np.array_equal(alone[key][0], mine), key
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["rows"][0], runs[50]["rows"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_events(x=None) are bit for bit what they
    are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
    dim = int(probs[0].dim_d)
    levels, side = np.stack([np.reshape(np.asarray(q.m0, dtype=float), dim) for q in probs]), sides_for(dim)

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_events(9, 4, levels, side=side, stride=2, prior=prior, per_particle=True) for step in order]
        if order[0] == "events":      # the cached x is the x: the same bits as with it given
            given = ctx.particle_events(9, 4, levels, side=side, stride=2, x=xs, prior=prior, per_particle=True)
            assert all(np.array_equal(given[key], out[0][key]) for key in given)
        ctx.close()
        return out

    a1, res, a2 = run(["record", "events", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["events", "record"])
    for key in res:
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    assert np.all(np.isfinite(res["mean"])) and np.all(np.diff(res["cdf"], axis=1) >= 0.0)


def test_records_of_vargp_and_problem_batch():
    v = build_problem("DW", "euler", 0.5)["vgp"]
    x = v.initialization()
    n_pts, dt = v.dim_n, float(v.fwd_ode.dt)
    rec = v.particle_events(300, 11, 0.0, side=-1, x=x, per_particle=True)
    assert isinstance(rec, va.PathEvents) and len(rec) == 300 and rec.rows.shape == (300, 3, 1) and rec.cdf.shape == (n_pts, 1)
    assert rec.n_pts == n_pts and rec.dt == dt and rec.stride == 1 and np.array_equal(rec.side, [-1]) and np.array_equal(rec.levels, [0.0])
    w = rec.weights()
    assert abs(rec.prob_crossed[0] - float(w @ (rec.rows[:, 1, 0] < n_pts))) <= 1e-12
    assert abs(rec.occupation_time[0] - dt * float(w @ rec.rows[:, 2, 0])) <= 1e-12 * max(1.0, rec.occupation_time[0])
    assert abs(rec.mean_extreme[0] - (0.0 - float(w @ rec.rows[:, 0, 0]))) <= 1e-12 * max(1.0, abs(rec.mean_extreme[0]))
    lo, hi = rec.extreme_quantile(0.1)[0], rec.extreme_quantile(0.9)[0]
    assert hi <= lo and -rec.rows[:, 0, 0].max() <= hi      # (side -1: the quantiles of the window's minimum, in the caller's units)
    flt = v.particle_filter(300, 11, x=x)
    assert np.array_equal(rec.log_w, flt.log_w) and rec.log_evidence() == flt.log_evidence()
    print("double well: P(x < 0 somewhere)", rec.prob_crossed, "median first passage", rec.first_passage_quantile(0.5),
          "occupation time", rec.occupation_time, "mean minimum", rec.mean_extreme)
    coarse = v.particle_events(300, 11, 0.0, side=-1, stride=7, x=x)
    assert coarse.rows is None and np.array_equal(coarse.cdf, rec.cdf[::7]) and np.array_equal(coarse.mean, rec.mean)
    pb = va.ProblemBatch([v])
    recs = pb.particle_events(300, 11, [[0.0]], side=[[-1]], x0=None, x=x, per_particle=True)
    pb.close()
    assert len(recs) == 1 and isinstance(recs[0], va.PathEvents)
    assert np.array_equal(recs[0].rows, rec.rows) and np.array_equal(recs[0].cdf, rec.cdf) and np.array_equal(recs[0].mean, rec.mean)
    assert np.array_equal(recs[0].ess, rec.ess) and np.array_equal(recs[0].resampled, rec.resampled)
    v.invalidate()


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    levels, side = 8.0 * np.ones((3, 12)), np.tile(sides_for(12), (3, 1))
    usable = lambda: ctx.particle_events(5, 1, levels, side=side, x=xs, prior=(mu, tau), per_particle=True)       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)                                               # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_events(5, 1, levels, side=side)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_events(0, 1, levels, side=side, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_events(bad, 1, levels, side=side, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_events(5, 1, levels, side=side, stride=bad, x=xs)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_events(5, 1, levels, side=side, stride=bad, x=xs)
    assert same(usable(), ref)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_events(5, 1, levels, side=side, ess_fraction=bad, x=xs)
    # through the C ABI itself: the outputs all null (one of them is enough), a side that is not +-1, a level that is not finite
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    rows, mean, cdf = np.empty((3, 5, 3, 12)), np.empty((3, 3, 12)), np.empty((3, ctx.Np, 12))
    sd = np.ascontiguousarray(side, dtype=np.int32)

    def call(a, b, c, lev=levels, sides=sd, stride=1):
        lev = np.ascontiguousarray(lev, dtype=float)
        return ctx._lib.vgpa_particle_events(ctx._h, xx.ctypes.data, None, 5, stride, 1, 0.5, None, None, lev.ctypes.data, sides.ctypes.data, lw.ctypes.data,
                                             st.ctypes.data, a, b, c, None, None)

    assert call(None, None, None) == -1 and b"rows, mean and cdf" in ctx._lib.vgpa_last_error(ctx._h)
    assert call(rows.ctypes.data, None, None) == 0 and call(None, mean.ctypes.data, None) == 0 and call(None, None, cdf.ctypes.data) == 0
    bare = ctx.particle_events(5, 1, levels, side=side, x=xs, per_particle=True)      # (no prior, as the calls above)
    assert np.array_equal(rows, bare["rows"]) and np.array_equal(mean, bare["mean"]) and np.array_equal(cdf, bare["cdf"])
    zero = sd.copy()
    zero[1, 3] = 0
    assert call(rows.ctypes.data, None, None, sides=zero) == -1 and b"+1 or -1" in ctx._lib.vgpa_last_error(ctx._h)
    for bad in (np.nan, np.inf):
        lev = levels.copy()
        lev[2, 11] = bad
        assert call(rows.ctypes.data, None, None, lev=lev) == -1 and b"finite" in ctx._lib.vgpa_last_error(ctx._h)
    assert call(rows.ctypes.data, None, None, stride=0) == -1 and b"stride" in ctx._lib.vgpa_last_error(ctx._h)
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
        ode.particle_events(2, 1, 0.0, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_events(2, 1, 8.0, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()
