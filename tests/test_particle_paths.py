"""
Whole smoothing trajectories from the particle filter's genealogy on the GPU (vgpa_particle_paths).

Two kinds of checks.
  The device against itself, which needs no margin: logw, state, ess and resampled are particle_filter's, bit for bit; at stride 1 every
  trajectory passes, bit for bit, through the filter's own cloud at every observation (paths[m][t_j] == clouds[j][slots[j][m]]) and ends
  in the filter's final particle (paths[m][Np-1] == state[slots[c][m]]); the slot table is the host trace of the device's own ancestors.
  Against the restatements of test_particle_paths_cpu: the device's histories are the restatement's (the margin conditions of
  test_particle_filter_cpu and test_particle_paths_cpu hold for every run here), so slots and resampled are compared exactly, and the
  paths with  |got - want| <= 1e-9 (scale + tiny)  entry by entry, scale = the largest |x| of the trajectory (what the rounding errors of
  its recursion are proportional to; conftest.rel_err's convention, taken per trajectory).  The reference walks the trajectories compared
  and no others (rewalk_numpy on the restatement's histories; test_trace_and_rewalk_is_the_forward_algorithm asserts that this is the
  forward algorithm's carried path, bit for bit); at most 65 of them per run.
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
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import (FRACTIONS, PLACEMENTS, SEED, SEED_BATCH, batch_case, case, particle_filter_numpy, placement_case)
from test_particle_filter_cpu import reference as filter_reference
from test_particle_paths_cpu import CASES, DRAWN, MARGIN, drawn_runs, pick_slots, rewalk_numpy, scale_of, trace_slots

pytestmark = pytest.mark.gpu

TOL = 1e-9
TINY = float(np.finfo(float).tiny)
WALK = ("log_w", "state", "ess", "resampled")
MOST = 65                 # trajectories the numpy reference walks per run
WORST = {"paths": 0.0}    # over the module, printed by the last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _against_itself(got, flt, obs_t, k=0, stride=1, label=""):
    """row k of Context.particle_paths' dict against row k of Context.particle_filter(history=True) with the same arguments"""
    c = len(obs_t)
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key][k], flt[key][k]), (label, key)
    table, paths = got["slots"][k], got["paths"][k]
    assert table.dtype == np.int32 and np.all(table[c + 1:] == -1), label
    table = table[:c + 1]
    n = flt["state"].shape[1]
    assert table.min() >= 0 and table.max() < n, label
    assert np.array_equal(table, trace_slots(table[c], flt["ancestors"][k, :c], flt["resampled"][k, :c])), label
    assert np.all(np.isfinite(paths))
    if stride == 1:
        for j, t in enumerate(obs_t):
            assert np.array_equal(paths[:, int(t)], flt["clouds"][k, j][table[j]]), (label, "observation", j)
        assert np.array_equal(paths[:, -1], flt["state"][k][table[c]]), (label, "the last point")


def _against_numpy(got, q, x, x0, seed, stride=1, k=0, index=None, label=""):
    """the first MOST trajectories of row k against the numpy walk of the device's own table (compared with the restatement's by the caller)"""
    c = int(np.asarray(q.obs_t).size)
    table = got["slots"][k, :c + 1, :MOST]
    want = rewalk_numpy(q, x, x0, seed, table, index=k if index is None else index)[:, ::stride]
    have = got["paths"][k, :MOST]
    assert have.shape == want.shape, (label, have.shape, want.shape)
    err = np.abs(have - want) / (scale_of(want) + TINY)
    WORST["paths"] = max(WORST["paths"], float(err.max()))
    print(label, f"stride {stride}: worst |got - want| / scale over {want.shape[0]} trajectories:", float(err.max()))
    assert np.all(np.abs(have - want) <= TOL * (scale_of(want) + TINY)), (label, float(err.max()))


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", [1, 17, 65, 300])
@pytest.mark.parametrize("tag,start", CASES)
def test_given_slots_every_lineage(contexts, tag, start, n_paths, ess_fraction):
    """slots = arange(n): every final slot's lineage.  D = 1, 1, 3, 12, 17, 40, 5, 64 (NT = 16, 32, 48, 64; 17 odd; 64 without a padding
    row); one lane, a partial wave, a partial 64-path block behind a full one, a second workgroup (a second 256-lane one at D <= 4);
    collapsed clouds (the fixtures) and the quiet cases' mix of resampled and carried clouds.  The device against itself, then slots,
    resampled and the first 65 trajectories against the restatement; a second call gives the same bits."""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    label = f"{tag} n={n_paths} {start} f={ess_fraction}"
    args = dict(ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    flt = ctx.particle_filter(n_paths, SEED, history=True, **args)
    got = ctx.particle_paths(n_paths, SEED, n_paths, slots=np.arange(n_paths), **args)
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    assert got["paths"].shape == (1, n_paths, int(q.n_pts), int(q.dim_d)) and got["slots"].shape == (1, obs_t.size + 1, n_paths)
    _against_itself(got, flt, obs_t, label=label)
    assert np.array_equal(got["slots"][0, -1], np.arange(n_paths))
    want = filter_reference(tag, start, n_paths, ess_fraction)
    assert np.array_equal(got["resampled"][0], want["resampled"]), label
    assert np.array_equal(got["slots"][0], trace_slots(np.arange(n_paths), want["ancestors"], want["resampled"])), label
    _against_numpy(got, q, x, s0, SEED, label=label)
    again = ctx.particle_paths(n_paths, SEED, n_paths, slots=np.arange(n_paths), **args)
    for key in got:
        assert np.array_equal(again[key], got[key]), (label, key)


@pytest.mark.parametrize("tag,start,n_paths,n_draw,ess_fraction", drawn_runs())
def test_drawn_slots(contexts, tag, start, n_paths, n_draw, ess_fraction):
    """the final slots drawn on the device from the final weights: exactly the restatement's (test_particle_paths_cpu.test_margin_condition
    clears every run listed here), K > n included; the device against itself; the trajectories against the restatement"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    label = f"{tag} n={n_paths} K={n_draw} {start} f={ess_fraction}"
    args = dict(ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    flt = ctx.particle_filter(n_paths, SEED, history=True, **args)
    got = ctx.particle_paths(n_paths, SEED, n_draw, **args)
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    _against_itself(got, flt, obs_t, label=label)
    want = filter_reference(tag, start, n_paths, ess_fraction)
    final, margin = pick_slots(want["lw"], n_draw, SEED, int(q.n_pts))
    assert margin >= MARGIN      # (the condition, once more where it is used)
    assert np.array_equal(got["slots"][0, -1], final), (label, got["slots"][0, -1], final)
    assert np.array_equal(got["slots"][0], trace_slots(final, want["ancestors"], want["resampled"])), label
    _against_numpy(got, q, x, s0, SEED, label=label)
    # the device's pick from the device's own weights, for good measure: the same slots
    assert np.array_equal(pick_slots(got["log_w"][0], n_draw, SEED, int(q.n_pts))[0], final), label


@pytest.mark.parametrize("n_paths", [17, 300])
@pytest.mark.parametrize("tag,start", CASES)
def test_against_the_moments_of_the_device(contexts, tag, start, n_paths):
    """two routes on the device: sum W paths and sum W paths^2 over every final slot's trajectory, W the normalised final weights, are
    particle_moments' M1 and M2 (which come from the descendant weights and the replay), to 1e-9 sum W |x| and 1e-9 M2, at strides 1, 4
    (kept indices on and off the observations) and Np + 3 (index 0 alone)"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    args = dict(ess_fraction=0.5, x=x, x0=x0 if start == "given" else None, prior=_prior(q))
    for stride in (1, 4, int(q.n_pts) + 3):
        got = ctx.particle_paths(n_paths, SEED, n_paths, stride=stride, slots=np.arange(n_paths), **args)
        mom = ctx.particle_moments(n_paths, SEED, stride=stride, **args)
        for key in WALK:
            assert np.array_equal(got[key], mom[key]), (tag, stride, key)
        w = np.exp(got["log_w"][0] - got["log_w"][0].max())
        w = w / w.sum()
        paths = got["paths"][0]
        assert paths.shape[1] == (int(q.n_pts) - 1) // stride + 1
        m1, m2, a1 = np.einsum("i,ikd->kd", w, paths), np.einsum("i,ikd->kd", w, paths * paths), np.einsum("i,ikd->kd", w, np.abs(paths))
        e1, e2 = np.abs(mom["moments"][0, :, 0] - m1), np.abs(mom["moments"][0, :, 1] - m2)
        print(tag, start, n_paths, f"stride {stride}: worst against particle_moments:", float(np.max(e1 / (a1 + TINY))), float(np.max(e2 / (m2 + TINY))))
        assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * m2), (tag, stride)
        if stride == 1:
            first = paths
        else:
            assert np.array_equal(paths, first[:, ::stride]), (tag, stride)


@pytest.mark.parametrize("tag,start", [c for c in CASES if not c[0].startswith("quiet")])
def test_without_resampling_it_is_the_sampler(contexts, tag, start):
    """ess_fraction = 0: no genealogy, trajectory m is row slots[m] of sample_paths with the same arguments, bit for bit -- for given slots
    (out of order, repeated) and for drawn ones"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    rows = ctx.sample_paths("posterior", 17, SEED, stride=3, x=x, x0=s0)[0]
    slots = np.array([16, 0, 5, 5, 11])
    got = ctx.particle_paths(17, SEED, 5, stride=3, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q), slots=slots)
    assert not got["resampled"].any() and np.all(got["slots"][0] == slots[None, :])
    assert np.array_equal(got["paths"][0], rows[slots]), (tag, start)
    drawn = ctx.particle_paths(17, SEED, 65, stride=3, ess_fraction=0.0, x=x, x0=s0, prior=_prior(q))
    assert np.all(drawn["slots"][0] == drawn["slots"][0, -1][None, :]) and np.array_equal(drawn["paths"][0], rows[drawn["slots"][0, -1]])


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (stretch 0 is the single index 0: the counter word changes before step 1), adjacent indices
    (stretches of one step), Np - 1 (an empty last stretch)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    obs_t = np.asarray(obs_at)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        label = f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}"
        args = dict(ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
        want = particle_filter_numpy(q, x, x0, 17, SEED, 1.0)
        flt = ctx.particle_filter(17, SEED, history=True, **args)
        got = ctx.particle_paths(17, SEED, 17, slots=np.arange(17), **args)
        _against_itself(got, flt, obs_t, label=label)
        assert np.array_equal(got["slots"][0], trace_slots(np.arange(17), want["ancestors"], want["resampled"])) and want["resampled"].any()
        _against_numpy(got, q, x, x0, SEED, label=label)
        final, margin = pick_slots(want["lw"], 65, SEED, int(q.n_pts))
        assert margin >= MARGIN, (label, margin)      # (the condition, for this case)
        for stride in (1, 4):
            got = ctx.particle_paths(17, SEED, 65, stride=stride, **args)
            _against_itself(got, flt, obs_t, stride=stride, label=label)
            assert np.array_equal(got["slots"][0, -1], final), label
            _against_numpy(got, q, x, x0, SEED, stride=stride, label=label)
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_no_observations(model, d):
    """a context without observations: one stretch, one row of slots, the sampler's paths of the picked slots"""
    q, x = placement_case(model, d, PLACEMENTS[0])
    q = dataclasses.replace(q, obs_t=np.zeros(0, dtype=np.int64), obs_y=np.zeros((0, d)))
    ctx = va.Context(model, "euler", d, int(q.n_pts), float(q.dt), sigma=q.sigma, theta=np.atleast_1d(q.theta), m0=q.m0, s0=q.s0)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    for s0 in (x0, None):
        got = ctx.particle_paths(17, SEED, 20, ess_fraction=0.5, x=x, x0=s0)
        flt = ctx.particle_filter(17, SEED, ess_fraction=0.5, x=x, x0=s0)
        rows = ctx.sample_paths("posterior", 17, SEED, x=x, x0=s0)[0]
        assert got["ess"].shape == (1, 0) and got["slots"].shape == (1, 1, 20)
        for key in WALK:
            assert np.array_equal(got[key], flt[key]), key
        final = pick_slots(got["log_w"][0], 20, SEED, int(q.n_pts))[0]      # (a given start: equal weights, thresholds (U + m) / 20 n against 1 .. n)
        assert np.array_equal(got["slots"][0, 0], final) and np.array_equal(got["paths"][0], rows[final])
        assert np.array_equal(got["paths"][0, :, -1], flt["state"][0][final])
        _against_numpy(got, q, x, s0, SEED, label=f"{model} no observations")
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with own theta, isotropic Sigma, observation times, counts, R and H: every lane switches its counter word at its own problem's
    observations (at D <= 4 the lanes of a wave belong to different problems); row k is the single-problem restatement of index k, and the
    last problem's result is bit for bit the same beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        args = dict(ess_fraction=0.5, x=xs, prior=prior)
        flt = ctx.particle_filter(40, SEED_BATCH, history=True, **args)
        given = ctx.particle_paths(40, SEED_BATCH, 40, slots=np.arange(40), **args)
        runs[first] = ctx.particle_paths(40, SEED_BATCH, 17, **args)
        third = ctx.particle_paths(40, SEED_BATCH, 17, stride=3, **args)
        own = ctx.particle_paths(40, SEED_BATCH, 2, slots=np.array([[0, 39], [5, 5], [39, 1]]), **args)
        ctx.close()
        assert np.array_equal(third["paths"], runs[first]["paths"][:, :, ::3]) and np.array_equal(third["slots"], runs[first]["slots"])
        for k, q in enumerate(probs):
            label = f"{model} batch {first} problem {k}"
            obs_t = np.asarray(q.obs_t, dtype=int).ravel()
            want = particle_filter_numpy(q, xs[k], None, 40, SEED_BATCH, 0.5, index=k)
            for res in (given, runs[first], own):
                _against_itself(res, flt, obs_t, k=k, label=label)
            final, margin = pick_slots(want["lw"], 17, SEED_BATCH, 41, index=k)
            assert margin >= MARGIN, (label, margin)      # (the condition, for this case)
            assert np.array_equal(given["slots"][k, :obs_t.size + 1], trace_slots(np.arange(40), want["ancestors"], want["resampled"])), label
            assert np.array_equal(runs[first]["slots"][k, :obs_t.size + 1], trace_slots(final, want["ancestors"], want["resampled"])), label
            assert np.array_equal(own["paths"][k], given["paths"][k][own["slots"][k, obs_t.size]]), label
            _against_numpy(given, q, xs[k], None, SEED_BATCH, k=k, label=label)
            _against_numpy(runs[first], q, xs[k], None, SEED_BATCH, k=k, label=label)
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["paths"][0], runs[50]["paths"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_paths(x=None) are bit for bit what
    they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_paths(9, 4, 9, prior=prior, slots=np.arange(9)) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "paths", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["paths", "record"])
    for key in res:
        assert np.array_equal(res[key], res_c[key]), key
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k
    k = nb - 1
    want = particle_filter_numpy(probs[k], xs[k], None, 9, 4, 0.5, index=k)      # (its margins: test_particle_moments_cpu clears this case)
    c = int(np.asarray(probs[k].obs_t).size)
    assert np.array_equal(res["slots"][k, :c + 1], trace_slots(np.arange(9), want["ancestors"], want["resampled"]))
    _against_numpy(res, probs[k], xs[k], None, 4, k=k, label=f"{name} cached x, problem {k}")


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_paths(5, 1, 7, x=xs, prior=(mu, tau))       # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)            # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_paths(5, 1, 7)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_paths(0, 1, 7, x=xs)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_draw"):
            ctx.particle_paths(5, 1, bad, x=xs)
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_paths(5, 1, 7, stride=bad, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_paths(5, 1, 7, stride=bad, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.particle_paths(5, 1, 2, x=xs, slots=[0, bad])
    assert ctx.particle_paths(5, 1, 7, stride=2 ** 31 - 1, x=xs)["paths"].shape == (3, 7, 1, 12)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_paths(5, 1, 7, ess_fraction=bad, x=xs)
    for bad in ([0, 5], [-1, 0], [[0, 1], [2, 3], [4, 7]]):      # a given slot outside [0, n)
        with pytest.raises(ValueError, match="final slot"):
            ctx.particle_paths(5, 1, 2, x=xs, slots=bad)
    assert same(usable(), ref)
    # through the C ABI itself: a null paths, logw or state; slots, ess and resampled are optional
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    pth = np.empty((3, 7, ctx.Np, 12))
    call = lambda n_draw, a, b, c: ctx._lib.vgpa_particle_paths(ctx._h, xx.ctypes.data, None, 5, n_draw, None, 1, 1, 0.5, None, None, a, b, c,      # noqa: E731
                                                                  None, None, None)
    assert call(7, lw.ctypes.data, st.ctypes.data, None) == -1
    assert call(7, None, st.ctypes.data, pth.ctypes.data) == -1 and call(7, lw.ctypes.data, None, pth.ctypes.data) == -1
    assert call(0, lw.ctypes.data, st.ctypes.data, pth.ctypes.data) == -1
    # more trajectories than the walk's grid.y holds: refused before any work (nothing is written)
    pth[:] = 3.0
    assert call(65535 * 64 + 1, lw.ctypes.data, st.ctypes.data, pth.ctypes.data) == -5
    assert b"trajectories are built for at most" in ctx._lib.vgpa_last_error(ctx._h) and np.all(pth == 3.0)
    assert call(7, lw.ctypes.data, st.ctypes.data, pth.ctypes.data) == 0
    assert np.array_equal(pth, ctx.particle_paths(5, 1, 7, x=xs)["paths"])
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
        ode.particle_paths(2, 1, 2, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_paths(2, 1, 2, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    # more entries than a result may have (at D <= 4 the walk's grid.x holds any int32 count): refused before any work
    q, x = placement_case("L63", 3, PLACEMENTS[0])
    small = gpu_context(q)
    xx, lw, st, pth = np.ascontiguousarray(x), np.empty((1, 5)), np.empty((1, 5, 3)), np.full((1, 2, 41, 3), 3.0)
    rc = small._lib.vgpa_particle_paths(small._h, xx.ctypes.data, None, 5, 2 ** 31 - 1, None, 1, 1, 0.5, None, None, lw.ctypes.data, st.ctypes.data,
                                        pth.ctypes.data, None, None, None)
    assert rc == -5 and b"2^35 entries" in small._lib.vgpa_last_error(small._h) and np.all(pth == 3.0)
    assert small.particle_paths(5, 1, 2, x=x)["paths"].shape == (1, 2, 41, 3)
    small.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_paths(2, 1, 2, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records_of_vargp_and_problem_batch():
    """ProblemBatch.particle_paths and VarGP.particle_paths: one SmoothingPaths per member, equal to the bare context's rows; the 1-D models
    drop the last axis"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.particle_paths(17, SEED_BATCH, 6, stride=2, x=x)
    given = pb.particle_paths(17, SEED_BATCH, 3, x=x, slots=[16, 0, 8])
    d = 12
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(3, d, d))
    bare = pb._context().particle_paths(17, SEED_BATCH, 6, stride=2, x=pb._stack(x), prior=prior)
    flt = pb._context().particle_filter(17, SEED_BATCH, x=pb._stack(x), prior=prior, history=True)
    pb.close()
    assert len(recs) == len(given) == 3
    for k, p in enumerate(ps):
        q = _fields(p["vgp"])
        want = particle_filter_numpy(q, x[k], None, 17, SEED_BATCH, 0.5, index=k)      # (its margins: test_particle_moments_cpu clears these members)
        final, margin = pick_slots(want["lw"], 6, SEED_BATCH, int(q.n_pts), index=k)
        assert margin >= MARGIN, (k, margin)      # (the condition, for these cases)
        rec = recs[k]
        c = rec.obs_t.size
        assert isinstance(rec, va.SmoothingPaths) and len(rec) == 6 and rec.stride == 2 and rec.drawn and not given[k].drawn
        assert np.array_equal(rec.paths, bare["paths"][k]) and np.array_equal(rec.log_w, bare["log_w"][k])
        assert np.array_equal(rec.slots, bare["slots"][k, :c + 1]) and np.array_equal(rec.slots, trace_slots(final, want["ancestors"], want["resampled"]))
        assert np.array_equal(rec.grid, np.arange(0, int(q.n_pts), 2)) and rec.mean().shape == rec.var().shape == (rec.grid.size, 12)
        assert np.all(np.diff(rec.distinct()) >= 0) and rec.distinct()[-1] == np.unique(final).size and np.isfinite(rec.log_evidence())
        assert rec.distinct_on_grid().shape == rec.grid.shape
        _against_itself(bare, flt, rec.obs_t, k=k, stride=2, label=f"ProblemBatch member {k}")
        _against_numpy(bare, q, x[k], None, SEED_BATCH, stride=2, k=k, label=f"ProblemBatch member {k}")
        assert np.array_equal(given[k].slots[-1], [16, 0, 8]) and np.array_equal(given[k].paths[:, -1], flt["state"][k][[16, 0, 8]])
        assert given[k].mean(given[k].final_weights()).shape == (int(q.n_pts), 12)
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.particle_paths(33, 3, 10, x=v.initialization())
    v.invalidate()
    assert rec.paths.shape == (10, v.dim_n) and rec.slots.shape == (rec.obs_t.size + 1, 10) and rec.mean().shape == rec.var().shape == (v.dim_n,)
    assert np.all(rec.var() >= 0.0) and 1 <= rec.distinct()[0] <= rec.distinct()[-1] <= 10


def test_report_worst_deviations():
    """No check of its own: prints the largest deviation the comparisons of this module have seen in this process so far (run behind them,
    the figure DESIGN.md s.4.13 quotes); every comparison asserts its own bound in _against_numpy."""
    print("worst |got - want| / scale of the trajectories over the module:", WORST)
