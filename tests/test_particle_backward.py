"""
Backward-simulation smoothing trajectories on the GPU (vgpa_particle_backward_paths).

Two kinds of checks, as in test_particle_paths.py.
  The device against itself, which needs no condition: logw, state, ess and resampled are particle_filter's, bit for bit; at stride 1 every
  trajectory passes, bit for bit, through the filter's own cloud at every observation (paths[m][t_j] == clouds[j][slots[j][m]]) and ends in
  the filter's final particle; two calls give the same bits; where nothing is resampled the result is particle_paths', bit for bit.
  Against the restatements of test_particle_backward_cpu: the filter's histories are the restatement's (the margin conditions of
  test_particle_filter_cpu and test_particle_paths_cpu hold for every run here) and every Gumbel-max draw keeps a gap >= 1e-8 between its two
  largest scores (test_particle_backward_cpu.test_gap_condition), four orders of magnitude over what the device's scores differ by, so the
  slot table is compared exactly; the paths with  |got - want| <= 1e-9 (scale + tiny)  entry by entry, scale = the largest |x| of the
  trajectory: the tolerance and scale of test_particle_paths.py.  The reference walks at most 65 trajectories per run.
Every grid has at most 101 points.
"""
import numpy as np
import pytest

import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_path_weights import _fields
from test_particle_filter import _batch_context, _ctx, _prior
from test_particle_filter_cpu import FRACTIONS, PLACEMENTS, SEED, SEED_BATCH, batch_case, case, placement_case
from test_particle_paths_cpu import DRAWN, MARGIN, pick_slots, scale_of
from test_particle_backward_cpu import (BCASES, BIG, GAP, TIGHT, TIGHT_RUNS, backward_runs, backward_slots_numpy, history, other_runs, reference,
                                        rewalk_backward_numpy, tight_case, tight_reference)

pytestmark = pytest.mark.gpu

TOL = 1e-9
TINY = float(np.finfo(float).tiny)
WALK = ("log_w", "state", "ess", "resampled")
MOST = 65                 # trajectories the numpy reference walks per run
WORST = {"paths": 0.0}    # over the module, printed behind its last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per case, closed behind the last test of the module (which also prints the largest deviation the comparisons of
    the module have seen; every comparison asserts its own bound in _against_numpy)"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()
    print("worst |got - want| / scale of the trajectories over the module:", WORST)


def _against_itself(got, flt, obs_t, k=0, stride=1, label=""):
    """row k of Context.particle_backward_paths' dict against row k of Context.particle_filter(history=True) with the same arguments"""
    c = len(obs_t)
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key][k], flt[key][k]), (label, key)
    table, paths = got["slots"][k], got["paths"][k]
    assert table.dtype == np.int32 and np.all(table[c + 1:] == -1), label
    table = table[:c + 1]
    n = flt["state"].shape[1]
    assert table.min() >= 0 and table.max() < n, label
    for j in range(c):      # (a cloud that was carried on leaves every trajectory in its slot)
        if not flt["resampled"][k, j]:
            assert np.array_equal(table[j], table[j + 1]), (label, j)
    assert np.all(np.isfinite(paths))
    if stride == 1:
        for j, t in enumerate(obs_t):
            assert np.array_equal(paths[:, int(t)], flt["clouds"][k, j][table[j]]), (label, "observation", j)
        assert np.array_equal(paths[:, -1], flt["state"][k][table[c]]), (label, "the last point")


def _against_numpy(got, q, x, x0, seed, hist, stride=1, k=0, index=None, label=""):
    """the first MOST trajectories of row k against the numpy walk of the device's own table (compared with the restatement's by the caller)"""
    c = int(np.asarray(q.obs_t).size)
    table = got["slots"][k, :c + 1, :MOST]
    want = rewalk_backward_numpy(q, x, x0, seed, table, hist, index=k if index is None else index)[:, ::stride]
    have = got["paths"][k, :MOST]
    assert have.shape == want.shape, (label, have.shape, want.shape)
    err = np.abs(have - want) / (scale_of(want) + TINY)
    WORST["paths"] = max(WORST["paths"], float(err.max()))
    print(label, f"stride {stride}: worst |got - want| / scale over {want.shape[0]} trajectories:", float(err.max()))
    assert np.all(np.abs(have - want) <= TOL * (scale_of(want) + TINY)), (label, float(err.max()))


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in a)


@pytest.mark.parametrize("tag,start,n_paths,n_draw,ess_fraction", backward_runs())
def test_drawn_slots(contexts, tag, start, n_paths, n_draw, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 64; one candidate, an odd candidate count, a partial wave, wave + 1, a second 256-slot tile; one trajectory
    and a second (partial) trajectory block behind full ones: the table is the restatement's, the device agrees with itself and with the
    restatement's walk, and a second call gives the same bits"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    label = f"{tag} n={n_paths} K={n_draw} {start} f={ess_fraction}"
    args = dict(ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    flt = ctx.particle_filter(n_paths, SEED, history=True, **args)
    got = ctx.particle_backward_paths(n_paths, SEED, n_draw, **args)
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    assert got["paths"].shape == (1, n_draw, int(q.n_pts), int(q.dim_d)) and got["slots"].shape == (1, obs_t.size + 1, n_draw)
    _against_itself(got, flt, obs_t, label=label)
    hist, final, table, gap = reference(tag, start, n_paths, n_draw, ess_fraction)
    assert gap >= GAP and pick_slots(hist["lw"], n_draw, SEED, int(q.n_pts))[1] >= MARGIN      # (the conditions, once more where they are used)
    assert np.array_equal(got["resampled"][0], hist["resampled"]), label
    assert np.array_equal(got["slots"][0], table), (label, np.argwhere(got["slots"][0] != table)[:4])
    _against_numpy(got, q, x, s0, SEED, hist, label=label)
    assert _same(ctx.particle_backward_paths(n_paths, SEED, n_draw, **args), got), label


@pytest.mark.parametrize("n_paths,n_draw", TIGHT_RUNS)
@pytest.mark.parametrize("d", TIGHT)
def test_tight_lorenz96_clouds(d, n_paths, n_draw):
    """Lorenz-96 where the draw decides (test_particle_backward_cpu.test_tight_clouds_react_to_the_kernel: the table is not the
    genealogy's and changes with a wrong drift): D = 12, 40 (one workgroup of the draw per compute unit) and 50 (NT = 64 with padding
    rows in the walk's reload).  The table is the restatement's, entry for entry"""
    q, x = tight_case(d)
    hist, final, table, gaps = tight_reference(d, n_paths, n_draw)
    assert min(float(g.min()) for g in gaps) >= GAP      # (the condition, once more where it is used)
    ctx = gpu_context(q)
    label = f"tight L96 D={d} n={n_paths} K={n_draw}"
    args = dict(ess_fraction=1.0, x=x, prior=_prior(q))
    flt = ctx.particle_filter(n_paths, SEED, history=True, **args)
    got = ctx.particle_backward_paths(n_paths, SEED, n_draw, **args)
    old = ctx.particle_paths(n_paths, SEED, n_draw, **args)
    ctx.close()
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    _against_itself(got, flt, obs_t, label=label)
    assert np.array_equal(got["resampled"][0], hist["resampled"]) and np.array_equal(got["slots"][0, -1], final), label
    assert np.array_equal(got["slots"][0], table), (label, np.argwhere(got["slots"][0] != table)[:4])
    assert not np.array_equal(got["slots"][0], old["slots"][0]), label
    _against_numpy(got, q, x, None, SEED, hist, label=label)


@pytest.mark.parametrize("tag,start", BCASES)
def test_without_resampling_it_is_the_genealogy(contexts, tag, start):
    """ess_fraction = 0, and one particle: nothing is resampled, no draw is made and the reload changes no bit -- particle_paths' result,
    for given slots (out of order, repeated) and drawn ones; and stride 3 is [::3] of stride 1 where draws are made"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    args = dict(x=x, x0=x0 if start == "given" else None, prior=_prior(q))
    slots = np.array([16, 0, 5, 5, 11])
    assert _same(ctx.particle_backward_paths(17, SEED, 5, stride=3, ess_fraction=0.0, slots=slots, **args),
                 ctx.particle_paths(17, SEED, 5, stride=3, ess_fraction=0.0, slots=slots, **args))
    assert _same(ctx.particle_backward_paths(17, SEED, 65, ess_fraction=0.0, **args), ctx.particle_paths(17, SEED, 65, ess_fraction=0.0, **args))
    assert _same(ctx.particle_backward_paths(1, SEED, 17, ess_fraction=1.0, **args), ctx.particle_paths(1, SEED, 17, ess_fraction=1.0, **args))
    one, third = ctx.particle_backward_paths(65, SEED, 17, ess_fraction=0.5, **args), ctx.particle_backward_paths(65, SEED, 17, stride=3, ess_fraction=0.5, **args)
    assert np.array_equal(third["paths"], one["paths"][:, :, ::3]) and np.array_equal(third["slots"], one["slots"])


@pytest.mark.parametrize("tag,start", [("ou_euler", "drawn"), ("l63_euler_p", "given"), ("l96d17_rk4_p", "drawn")])
def test_given_final_slots(contexts, tag, start):
    """the caller's final slots (out of order, repeated) in place of drawn ones: the table is the restatement's from those slots, and a
    trajectory's draws depend on its own index and final slot only -- trajectory 2 of five is trajectory 2 of seventy"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    args = dict(ess_fraction=0.5, x=x, x0=s0, prior=_prior(q))
    slots = np.array([64, 0, 5, 5, 11])
    flt = ctx.particle_filter(65, SEED, history=True, **args)
    got = ctx.particle_backward_paths(65, SEED, 5, slots=slots, **args)
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    _against_itself(got, flt, obs_t, label=tag)
    hist = history(tag, start, 65, 0.5)
    table, gaps = backward_slots_numpy(q, x, SEED, hist, slots)
    assert min(float(g.min()) for g in gaps) >= GAP      # (the condition, for this case)
    assert np.array_equal(got["slots"][0], table) and np.array_equal(got["slots"][0, -1], slots)
    _against_numpy(got, q, x, s0, SEED, hist, label=f"{tag} given slots")
    wide = ctx.particle_backward_paths(65, SEED, 70, slots=np.concatenate((slots, np.arange(65))), **args)
    assert np.array_equal(wide["paths"][0, :5], got["paths"][0]) and np.array_equal(wide["slots"][0, :, :5], got["slots"][0])


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (the reload comes before step 1), adjacent indices (stretches of one step), Np - 1 (an empty last
    stretch, where nothing is resampled)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    obs_t = np.asarray(obs_at)
    runs = {r[0]: r for r in other_runs()}
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        label = f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}"
        _, _, _, _, _, _, hist, final = runs[(model, obs_at, x0 is None)]
        args = dict(ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
        flt = ctx.particle_filter(17, SEED, history=True, **args)
        table, gaps = backward_slots_numpy(q, x, SEED, hist, final)
        assert hist["resampled"].any() and min(float(g.min()) for g in gaps) >= GAP, label
        for stride in (1, 4):
            got = ctx.particle_backward_paths(17, SEED, 65, stride=stride, **args)
            _against_itself(got, flt, obs_t, stride=stride, label=label)
            assert np.array_equal(got["slots"][0], table), label
            _against_numpy(got, q, x, x0, SEED, hist, stride=stride, label=label)
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with own theta, isotropic Sigma, observation times, counts, R and H: every workgroup walks its own problem's cuts with that
    problem's theta and Sigma; row k is the single-problem restatement of index k, rows beyond a problem's count + 1 are -1, and the last
    problem's result is bit for bit the same beside two other neighbours"""
    runs, refs = {}, {r[0]: r for r in other_runs()}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        args = dict(ess_fraction=0.5, x=xs, prior=prior)
        flt = ctx.particle_filter(40, SEED_BATCH, history=True, **args)
        runs[first] = ctx.particle_backward_paths(40, SEED_BATCH, 17, **args)
        ctx.close()
        for k, q in enumerate(probs):
            label = f"{model} batch {first} problem {k}"
            obs_t = np.asarray(q.obs_t, dtype=int).ravel()
            _, _, _, _, _, _, hist, final = refs[(model, "batch", first, k)]
            _against_itself(runs[first], flt, obs_t, k=k, label=label)
            table, gaps = backward_slots_numpy(q, xs[k], SEED_BATCH, hist, final, index=k)
            assert min([float(g.min()) for g in gaps], default=np.inf) >= GAP, label
            assert np.array_equal(runs[first]["slots"][k, :obs_t.size + 1], table), label
            _against_numpy(runs[first], q, xs[k], None, SEED_BATCH, hist, k=k, label=label)
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["paths"][0], runs[50]["paths"][0])


def test_records_of_vargp_and_problem_batch():
    """ProblemBatch.backward_paths and VarGP.backward_paths: one SmoothingPaths with method "backward" per member, equal to the bare
    context's rows; the 1-D models drop the last axis"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.backward_paths(17, SEED_BATCH, 6, stride=2, x=x)
    given = pb.backward_paths(17, SEED_BATCH, 3, x=x, slots=[16, 0, 8])
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(3, 12, 12))
    bare = pb._context().particle_backward_paths(17, SEED_BATCH, 6, stride=2, x=pb._stack(x), prior=prior)
    flt = pb._context().particle_filter(17, SEED_BATCH, x=pb._stack(x), prior=prior, history=True)
    pb.close()
    refs = {r[0]: r for r in other_runs()}
    assert len(recs) == len(given) == 3
    for k, p in enumerate(ps):
        q = _fields(p["vgp"])
        _, _, _, _, _, _, hist, final = refs[("member", k)]
        table, gaps = backward_slots_numpy(q, x[k], SEED_BATCH, hist, final, index=k)
        assert min([float(g.min()) for g in gaps], default=np.inf) >= GAP, k
        rec = recs[k]
        c = rec.obs_t.size
        assert isinstance(rec, va.SmoothingPaths) and rec.method == "backward" and len(rec) == 6 and rec.stride == 2 and rec.drawn and not given[k].drawn
        assert np.array_equal(rec.paths, bare["paths"][k]) and np.array_equal(rec.log_w, bare["log_w"][k])
        assert np.array_equal(rec.slots, bare["slots"][k, :c + 1]) and np.array_equal(rec.slots, table)
        assert rec.mean().shape == rec.var().shape == (rec.grid.size, 12) and rec.distinct()[-1] == np.unique(final).size
        _against_itself(bare, flt, rec.obs_t, k=k, stride=2, label=f"ProblemBatch member {k}")
        _against_numpy(bare, q, x[k], None, SEED_BATCH, hist, stride=2, k=k, label=f"ProblemBatch member {k}")
        assert given[k].method == "backward" and np.array_equal(given[k].slots[-1], [16, 0, 8])
        assert np.array_equal(given[k].paths[:, -1], flt["state"][k][[16, 0, 8]])
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.backward_paths(33, 3, 10, x=v.initialization())
    old = v.particle_paths(33, 3, 10, x=v.initialization())
    v.invalidate()
    assert rec.method == "backward" and old.method == "genealogy" and rec.paths.shape == (10, v.dim_n) and rec.slots.shape == (rec.obs_t.size + 1, 10)
    assert np.array_equal(rec.slots[-1], old.slots[-1]) and np.array_equal(rec.log_w, old.log_w) and np.all(rec.var() >= 0.0)


def test_errors():
    """the refusals of particle_paths: a dense Sigma, D > 64, an ODE-only context, no model; the context stays usable afterwards"""
    from test_problem_batch import _context, _datasets
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_backward_paths(5, 1, 7, x=xs, prior=(mu, tau))       # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_backward_paths(5, 1, 7)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.particle_backward_paths(0, 1, 7, x=xs)
    with pytest.raises(ValueError, match="n_draw"):
        ctx.particle_backward_paths(5, 1, 0, x=xs)
    with pytest.raises(ValueError, match="stride"):
        ctx.particle_backward_paths(5, 1, 7, stride=0, x=xs)
    with pytest.raises(ValueError, match="final slot"):
        ctx.particle_backward_paths(5, 1, 2, x=xs, slots=[0, 5])
    assert _same(usable(), ref)
    # through the C ABI itself: a null paths; more trajectories than the draw's grid.y holds: refused before any work (nothing is written)
    xx, lw, st, pth = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12)), np.full((3, 7, ctx.Np, 12), 3.0)
    call = lambda n_draw, a: ctx._lib.vgpa_particle_backward_paths(ctx._h, xx.ctypes.data, None, 5, n_draw, None, 1, 1, 0.5, None, None,      # noqa: E731
                                                                     lw.ctypes.data, st.ctypes.data, a, None, None, None)
    assert call(7, None) == -1
    assert call(65535 * 8 + 1, pth.ctypes.data) == -5
    assert b"backward simulation is built for at most" in ctx._lib.vgpa_last_error(ctx._h) and np.all(pth == 3.0)
    assert call(7, pth.ctypes.data) == 0 and np.array_equal(pth, ctx.particle_backward_paths(5, 1, 7, x=xs)["paths"])
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert _same(usable(), ref)
    ctx.close()
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_backward_paths(2, 1, 2, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_backward_paths(2, 1, 2, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_backward_paths(2, 1, 2, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_large_run_keeps_more_distinct_paths(contexts):
    """ou_euler at 4096 particles and 4096 trajectories (16 tiles of candidates, 512 trajectory blocks), the final slots given as the
    restatement picks them: the table is the restatement's, and the first stretch holds more distinct paths than particle_paths leaves on
    the same run"""
    tag, n, k, frac, seed = BIG
    q, x, _ = case(tag)
    ctx = _ctx(contexts, tag)
    hist, final, table, gap = reference(tag, "drawn", n, k, frac, seed)
    assert gap >= GAP
    args = dict(ess_fraction=frac, x=x, prior=_prior(q), slots=final)
    got, old = ctx.particle_backward_paths(n, seed, k, **args), ctx.particle_paths(n, seed, k, **args)
    assert np.array_equal(got["resampled"][0], hist["resampled"]) and hist["resampled"].any()
    assert np.array_equal(got["slots"][0], table), np.argwhere(got["slots"][0] != table)[:4]
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    recs = [va.SmoothingPaths(r["log_w"][0], r["paths"][0], r["slots"][0], 1, int(q.n_pts), obs_t, drawn=False, method=m)
            for r, m in ((got, "backward"), (old, "genealogy"))]
    print("distinct paths per stretch: backward", recs[0].distinct(), "genealogy", recs[1].distinct())
    assert recs[0].distinct_on_grid()[0] > recs[1].distinct_on_grid()[0]
    _against_numpy(got, q, x, None, seed, hist, label="ou_euler 4096 x 4096")
