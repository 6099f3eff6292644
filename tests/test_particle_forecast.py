"""
The particle forecast on the GPU (vgpa_particle_forecast).

Against the restatement test_particle_forecast_cpu.forecast_numpy: moments, members and the end state with conftest.rel_err <= 1e-9 (the
walk is at most 40 steps of the same operations in the same association; the moments are sums of at most 300 terms of one sign for M2
and of the states' own size for M1).  Drawn slots are compared exactly: test_particle_forecast_cpu.test_margin_condition clears every
pick made here.  The device against itself needs no margin: behind the filter log_w, state, ess and resampled are particle_filter's bit
for bit, member m at h = 0 is the last point of trajectory m of particle_paths bit for bit, a member is its slot of the whole cloud, and a
forecast split in two arrives at the same bits.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from conftest import rel_err
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights import _fields
from test_particle_filter import CACHE_CASES, _ctx, _prior
from test_particle_filter_cpu import MARGIN, SEED, SEED_BATCH, case
from test_particle_filter_cpu import reference as filter_reference
from test_particle_forecast_cpu import BEHIND, DRAWN, FC_SEED, SHAPES, SIZES, STEPS, WEIGHTS, cloud_case, forecast_numpy, shape_problem
from test_particle_paths_cpu import pick_slots

pytestmark = pytest.mark.gpu

TOL = 1e-9
WALK = ("log_w", "state", "ess", "resampled")
WORST = {"moments": 0.0, "members": 0.0, "state_end": 0.0}      # over the module, printed by the last test


@pytest.fixture(scope="module")
def contexts():
    """one bare context per shape or case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _shape_ctx(cache, model, d):
    if (model, d) not in cache:
        cache[(model, d)] = gpu_context(shape_problem(model, d))
    return cache[(model, d)]


def _compare(got, want, k=0, label=""):
    """row k of Context.particle_forecast's dict against one restatement"""
    for key in ("moments", "members", "state_end"):
        assert got[key][k].shape == want[key].shape, (label, key, got[key][k].shape, want[key].shape)
        assert np.all(np.isfinite(got[key][k])), (label, key)
        err = rel_err(got[key][k], want[key])
        WORST[key] = max(WORST[key], err)
        assert err <= TOL, (label, key, err)
    assert got["slots"].dtype == np.int32 and np.array_equal(got["slots"][k], want["slots"]), (label, got["slots"][k], want["slots"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("model,d", SHAPES, ids=lambda v: str(v))
def test_given_cloud_against_numpy(contexts, model, d, n):
    """every (horizon, stride, index0) of STEPS and every kind of weights, with given slots (out of order, repeated): moments, members,
    end state; the log-weights and the cloud come back as they went in.  The contexts have evaluated nothing."""
    q, ctx = shape_problem(model, d), _shape_ctx(contexts, model, d)
    slots = np.array([n - 1, 0, n // 2, n // 2, min(n - 1, 64)])
    for horizon, stride, index0 in STEPS:
        for weights in WEIGHTS:
            cloud, lw = cloud_case(model, d, n, weights)
            label = f"{model} D={d} n={n} H={horizon} stride={stride} k0={index0} {weights}"
            got = ctx.particle_forecast(horizon, seed=FC_SEED, stride=stride, n_draw=slots.size, cloud=cloud, log_w=lw, index0=index0, slots=slots)
            _compare(got, forecast_numpy(q, cloud, lw, index0, horizon, stride, FC_SEED, slots), label=label)
            assert np.array_equal(got["state"][0], cloud) and got["index0"] == index0 and got["ess"] is None
            assert np.array_equal(got["log_w"][0], np.zeros(n) if lw is None else lw)
            if horizon == 0:
                assert np.array_equal(got["state_end"][0], cloud) and np.array_equal(got["members"][0, :, 0], cloud[slots]), label
    print(model, d, n, "worst rel_err so far:", WORST)


@pytest.mark.parametrize("model,d,n,k,weights", DRAWN, ids=lambda v: str(v))
def test_drawn_slots_on_a_given_cloud(contexts, model, d, n, k, weights):
    """the slots drawn on the device from the given weights are the restatement's (K > n included), the members are their slots of the
    whole cloud, bit for bit, and a second call gives the same bits"""
    q, ctx = shape_problem(model, d), _shape_ctx(contexts, model, d)
    cloud, lw = cloud_case(model, d, n, weights)
    label = f"{model} D={d} n={n} K={k} {weights}"
    want = forecast_numpy(q, cloud, lw, 40, 7, 3, FC_SEED, k)
    assert want["margin"] >= MARGIN      # (the condition, once more where it is used)
    got = ctx.particle_forecast(7, seed=FC_SEED, stride=3, n_draw=k, cloud=cloud, log_w=lw)
    assert got["index0"] == 40
    _compare(got, want, label=label)
    every = ctx.particle_forecast(7, seed=FC_SEED, stride=3, n_draw=n, cloud=cloud, log_w=lw, index0=40, slots=np.arange(n))
    assert np.array_equal(got["members"][0], every["members"][0][want["slots"]]), label
    assert np.array_equal(every["members"][0][:, 0], cloud), label
    for key in ("moments", "state_end"):
        assert np.array_equal(got[key], every[key]), (label, key)
    again = ctx.particle_forecast(7, seed=FC_SEED, stride=3, n_draw=k, cloud=cloud, log_w=lw)
    for key in ("moments", "members", "slots", "state_end"):
        assert np.array_equal(again[key], got[key]), (label, key)
    none = ctx.particle_forecast(7, seed=FC_SEED, stride=3, cloud=cloud, log_w=lw)
    assert none["members"].shape == (1, 0, 3, d) and none["slots"].shape == (1, 0) and np.array_equal(none["moments"], got["moments"])


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with per-problem theta and Sigma, own clouds and weights; 65 particles: at D <= 4 the 256 lanes of a workgroup belong to one
    problem, above it a problem has a full and a partial workgroup.  Problem p draws with the counter word p."""
    q0 = shape_problem(model, d)
    probs = [dataclasses.replace(q0, theta=np.asarray(q0.theta, dtype=float) * (1.0 + 0.05 * p) if model == "L63" else float(q0.theta) * (1.0 + 0.05 * p),
                                 sigma=np.asarray(q0.sigma) * (1.0 + 0.2 * p)) for p in range(3)]
    ctx = gpu_context(q0, batch=3)
    ctx.set_problem_params(theta=np.stack([np.atleast_1d(q.theta) for q in probs]), sigma=np.stack([q.sigma for q in probs]))
    clouds = np.stack([cloud_case(model, d, 65, "random", p)[0] for p in range(3)])
    lws = np.stack([cloud_case(model, d, 65, "random", p)[1] for p in range(3)])
    got = ctx.particle_forecast(7, seed=FC_SEED, stride=3, n_draw=17, cloud=clouds, log_w=lws, index0=40)
    shared = ctx.particle_forecast(7, seed=FC_SEED, stride=3, n_draw=17, cloud=clouds[0], log_w=lws[0], index0=40)
    ctx.close()
    for p, q in enumerate(probs):
        want = forecast_numpy(q, clouds[p], lws[p], 40, 7, 3, FC_SEED, 17, index=p)
        assert want["margin"] >= MARGIN
        _compare(got, want, k=p, label=f"{model} batch problem {p}")
    # a cloud without a batch axis is every problem's; the problems still differ (theta, Sigma, the counter word)
    assert np.array_equal(shared["moments"][0], got["moments"][0]) and not np.array_equal(shared["state_end"][1], shared["state_end"][0])


@pytest.mark.parametrize("model,d", SHAPES, ids=lambda v: str(v))
def test_splitting(contexts, model, d):
    """12 steps = 6 steps, then 6 from the end state with index0 + 6: the end states bit for bit; moments and members at TOL"""
    ctx = _shape_ctx(contexts, model, d)
    cloud, lw = cloud_case(model, d, 65, "random")
    slots = np.array([64, 0, 5, 5])
    args = dict(seed=FC_SEED, stride=3, n_draw=4, log_w=lw, slots=slots)
    whole = ctx.particle_forecast(12, cloud=cloud, index0=33, **args)
    first = ctx.particle_forecast(6, cloud=cloud, index0=33, **args)
    rest = ctx.particle_forecast(6, cloud=first["state_end"], index0=39, **args)
    assert np.array_equal(rest["state_end"], whole["state_end"]), (model, d)
    assert rel_err(np.concatenate((first["moments"], rest["moments"][:, 1:]), axis=1), whole["moments"]) <= TOL
    assert rel_err(np.concatenate((first["members"], rest["members"][:, :, 1:]), axis=2), whole["members"]) <= TOL
    other = ctx.particle_forecast(6, cloud=first["state_end"], index0=38, **args)
    assert not np.array_equal(other["state_end"], whole["state_end"])      # (the absolute grid index is in the counter)


@pytest.mark.parametrize("model,d", [("OU", 1), ("DW", 1), ("L63", 3), ("L96", 4), ("L96", 5), ("L96", 40)], ids=lambda v: str(v))
def test_agreement_with_the_model_sampler(contexts, model, d):
    """a cloud of n copies of x0, index0 = 0, H = Np - 1, slots 0 .. n-1: the members are sample_paths("model", x0=x0)"""
    q, ctx = shape_problem(model, d), _shape_ctx(contexts, model, d)
    x0 = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    for n, stride in ((17, 1), (65, 4)):
        want = ctx.sample_paths("model", n, FC_SEED, stride=stride, x0=x0)
        got = ctx.particle_forecast(int(q.n_pts) - 1, seed=FC_SEED, stride=stride, n_draw=n, cloud=np.tile(x0, (n, 1)), index0=0, slots=np.arange(n))
        assert got["members"].shape == want.shape
        err = rel_err(got["members"], want)
        print(model, d, n, "against the model-kind sampler:", err)
        assert err <= TOL, (model, d, n, err)
        assert rel_err(got["state_end"][0], want[0, :, -1]) <= TOL      # (both strides divide Np - 1 = 40)
        assert rel_err(got["moments"][0, :, 0], want[0].mean(axis=0)) <= TOL


@pytest.mark.parametrize("tag,start,n,k", BEHIND, ids=lambda v: str(v))
def test_behind_the_filter(contexts, tag, start, n, k):
    """log_w, state, ess, resampled are particle_filter's bit for bit; the forecast from them agrees with the restatement; the drawn slots
    are those of particle_paths, whose trajectories the members continue: member m at h = 0 is its last point, bit for bit"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    label = f"{tag} n={n} K={k} {start}"
    args = dict(ess_fraction=0.5, x=x, x0=s0, prior=_prior(q))
    flt = ctx.particle_filter(n, SEED, **args)
    got = ctx.particle_forecast(7, n, SEED, stride=3, n_draw=k, **args)
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), (label, key)
    last = int(q.n_pts) - 1
    assert got["index0"] == last
    final, margin = pick_slots(filter_reference(tag, start, n, 0.5)["lw"], k, SEED, last + 1)
    assert margin >= MARGIN      # (the condition, once more where it is used)
    assert np.array_equal(got["slots"][0], final), (label, got["slots"][0], final)
    _compare(got, forecast_numpy(q, got["state"][0], got["log_w"][0], last, 7, 3, SEED, final), label=label)
    paths = ctx.particle_paths(n, SEED, k, stride=last, **args)
    assert np.array_equal(paths["slots"][0, np.asarray(q.obs_t).size], got["slots"][0]), label
    assert np.array_equal(got["members"][0, :, 0], paths["paths"][0, :, -1]), (label, "continuation")
    assert np.array_equal(got["members"][0, :, 0], got["state"][0][final]), label
    again = ctx.particle_forecast(7, n, SEED, stride=3, n_draw=k, **args)
    for key in got:
        assert np.array_equal(again[key], got[key]), (label, key)


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_forecast(x=None), behind the filter and
    from a given cloud, are bit for bit what they are without the call"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
    cloud = 1.0 + np.random.default_rng(2).standard_normal((nb, 9, probs[0].dim_d))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def forecast(ctx):
        return ctx.particle_forecast(5, 9, 4, stride=2, n_draw=3, prior=prior), ctx.particle_forecast(5, seed=4, n_draw=3, cloud=cloud)

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else forecast(ctx) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "forecast", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["forecast", "record"])
    for one, two in zip(res, res_c):
        for key in ("log_w", "state", "moments", "members", "slots", "state_end"):
            assert np.array_equal(one[key], two[key]), key
        assert np.all(np.isfinite(one["moments"]))
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k


def test_errors():
    q = shape_problem("L96", 12)
    ctx = gpu_context(q)
    cloud, lw = cloud_case("L96", 12, 17, "random")
    usable = lambda: ctx.particle_forecast(3, seed=1, n_draw=2, cloud=cloud, log_w=lw)      # noqa: E731
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ("moments", "members", "slots", "state_end"))      # noqa: E731
    ref = usable()
    for bad in (dict(horizon=-1), dict(stride=0), dict(n_draw=-1), dict(index0=-1), dict(index0=2 ** 31 - 3), dict(slots=np.array([0, 17])),
                dict(slots=np.array([-1, 0]))):
        args = dict(horizon=3, seed=1, n_draw=2, cloud=cloud, log_w=lw)
        args.update(bad)
        with pytest.raises(ValueError):
            ctx.particle_forecast(**args)
    with pytest.raises(ValueError):      # drawn slots take their uniform from index0 + 1
        ctx.particle_forecast(0, seed=1, n_draw=2, cloud=cloud, index0=2 ** 31 - 1)
    assert ctx.particle_forecast(0, seed=1, n_draw=2, cloud=cloud, index0=2 ** 31 - 1, slots=np.array([0, 16]))["moments"].shape == (1, 1, 2, 12)
    with pytest.raises(ValueError):
        ctx.particle_forecast(3, n_paths=5, cloud=cloud)
    with pytest.raises(ValueError):
        ctx.particle_forecast(3)
    with pytest.raises(RuntimeError, match="no cached state"):      # the filter's errors, behind the filter
        ctx.particle_forecast(3, 5, 1)
    # through the C ABI itself: a null moments
    st = np.empty((1, 17, 12))
    assert ctx._lib.vgpa_particle_forecast(ctx._h, None, None, 17, 1, 0.5, None, None, cloud.ctypes.data, None, 40, 3, 1, 0, None, None, None,
                                           None, None, None, None, None, st.ctypes.data) == -1
    assert same(usable(), ref)
    # a dense Sigma in force
    ctx.set_problem_params(sigma=(np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)))[None])
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.reshape(q.sigma, (12, 12))[None])
    assert same(usable(), ref)
    ctx.close()
    # no model: ValueError
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_forecast(3, cloud=np.ones((2, 5, 3)))
    ode.close()
    # a model without prior moments and observations: a given cloud is all the forecast needs; the filter is refused
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    assert np.all(np.isfinite(bare.particle_forecast(3, seed=1, cloud=np.ones((2, 5, 3)))["moments"]))
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_forecast(3, 2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    # D > 64
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_forecast(3, cloud=np.ones((4, 72)))
    with pytest.raises(NotImplementedError):
        big.particle_forecast(3, 2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records():
    """VarGP.forecast and ProblemBatch.forecast: one record per member, behind the filter, from the posterior process's end points and
    from the state of an earlier forecast"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.forecast(6, 17, SEED_BATCH, stride=2, n_draw=3, x=x)
    flt = pb.particle_filter(17, SEED_BATCH, x=x)
    post = pb.forecast(6, 17, SEED_BATCH, stride=2, n_draw=3, x=x, source="posterior")
    ends = pb.sample_paths(17, SEED_BATCH, stride=ps[0]["vgp"].dim_n - 1, x=x)[:, :, -1]
    on = pb.forecast(4, seed=SEED_BATCH, cloud=np.stack([r.state for r in recs]), log_w=np.stack([r.log_w for r in recs]), index0=int(recs[0].grid[-1]))
    whole = pb.forecast(10, 17, SEED_BATCH, x=x)
    pb.close()
    assert len(recs) == len(post) == 3
    for k, p in enumerate(ps):
        v, rec = p["vgp"], recs[k]
        last = v.dim_n - 1
        assert isinstance(rec, va.Forecast) and len(rec) == 17 and rec.stride == 2 and rec.drawn
        assert np.array_equal(rec.grid, last + np.array([0, 2, 4, 6])) and np.allclose(rec.times, v.model.time_window[0] + float(v.fwd_ode.dt) * rec.grid)
        assert np.array_equal(rec.log_w, flt[k].log_w) and np.array_equal(rec.members[:, 0], flt[k].state[rec.slots])
        want = forecast_numpy(_fields(v), flt[k].state, flt[k].log_w, last, 6, 2, SEED_BATCH, rec.slots, index=k)
        assert rel_err(rec.mean, want["moments"][:, 0]) <= TOL and rel_err(rec.members, want["members"]) <= TOL and rel_err(rec.state, want["state_end"]) <= TOL
        assert rec.var.shape == (4, 12) and np.all(rec.var >= 0.0)
        assert np.array_equal(rec.var, np.maximum(rec.moments[:, 1] - rec.moments[:, 0] ** 2, 0.0))
        # the posterior process's end points, equally weighted
        want = forecast_numpy(_fields(v), ends[k], None, last, 6, 2, SEED_BATCH, post[k].slots, index=k)
        assert np.array_equal(post[k].log_w, np.zeros(17)) and np.array_equal(post[k].members[:, 0], ends[k][post[k].slots])
        assert rel_err(post[k].mean, want["moments"][:, 0]) <= TOL and rel_err(post[k].state, want["state_end"]) <= TOL
        # a forecast goes on from the record of the one before it
        assert np.array_equal(on[k].state, whole[k].state) and np.array_equal(on[k].grid, last + 6 + np.arange(5))
    # one VarGP of the 1-D models: the last axis is dropped
    v = build_problem("OU", "euler", 0.5)["vgp"]
    xi = v.initialization()
    rec = v.forecast(5, 33, 3, n_draw=4, x=xi)
    post = v.forecast(5, 33, 3, x=xi, source="posterior")
    on = v.forecast(2, seed=3, cloud=rec.state, log_w=rec.log_w, index0=int(rec.grid[-1]), slots=[0, 32])
    v.invalidate()
    assert rec.mean.shape == (6,) and rec.var.shape == (6,) and rec.members.shape == (4, 6) and rec.state.shape == (33,) and rec.slots.shape == (4,)
    assert post.members.shape == (0, 6) and len(post) == 33 and on.members.shape == (2, 3) and not on.drawn
    print("worst rel_err over the module:", WORST)
