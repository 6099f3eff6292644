"""
Importance weights of sampled posterior paths on the GPU (vgpa_sample_paths_weighted).

Reference: test_path_weights_cpu.path_weights_numpy, evaluated with each problem's own rows.  Tolerance, per path and per term:
|got - want| <= 1e-9 (1 + scale), scale = sum_k |increment_k| of the path term; 1e-9 is the suite's TOL on the paths these sums are built
from.  Every grid has at most 101 points.

(Lorenz-96 at D = 5 comes from test_gpu_edge_cases.make_problem on a bare context, as in test_sample_paths.py.)
"""
import dataclasses
import types

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd.weights import init_term
from conftest import load_golden, rel_err
from helpers import build_problem, problem_from_golden
from test_gpu_edge_cases import gpu_context, make_problem, spd
from test_problem_batch import _context, _datasets
from test_path_weights_cpu import FIXTURES, TAGS, independent_form, path_weights_numpy

pytestmark = pytest.mark.gpu

TOL = 1e-9
N_MAX = 65


def _excess(got, want, scale):
    """max over paths of |got - want| / (1 + scale); a NaN stays a NaN"""
    return float(np.max(np.maximum(np.abs(np.asarray(got) - np.asarray(want)) / (1.0 + scale), 0.0)))


def _fields(vgp):
    """what the numpy restatement reads of one VarGP: its inputs NOW and its prior"""
    inp = vgp._inputs()
    return types.SimpleNamespace(model=vgp.model._model_id, dim_d=vgp.dim_d, n_pts=vgp.dim_n, dt=float(vgp.fwd_ode.dt),
                                 theta=inp["theta"] if inp["theta"].size > 1 else float(inp["theta"][0]), sigma=inp["sigma"],
                                 m0=inp["m0"], s0=inp["s0"], mu0=vgp.kl0.mu0, tau0=vgp.kl0.tau0, obs_t=inp["obs_t"], obs_y=inp["obs_y"],
                                 obs_noise=inp["obs_noise"], obs_h=inp["obs_h"])


@pytest.fixture(scope="module")
def cases():
    """the problems and their numpy references at N_MAX paths, built once per tag / start and shared by the tests of this module (path i
    does not depend on n_paths); the contexts are closed behind the last test"""
    cache = {}
    yield cache
    for key, val in cache.items():
        if isinstance(key, str) and val[0] is not None:
            val[0].invalidate()


def _case(cache, tag):
    """(VarGP or None, fields, x)"""
    if tag not in cache:
        if tag in FIXTURES:
            z = load_golden(tag)
            v = problem_from_golden(z)["vgp"]
            cache[tag] = (v, _fields(v), np.asarray(z["x"], dtype=float))
        elif tag == "l96d64":
            v = build_problem("L96", "euler", 0.5, dim_d=64)["vgp"]
            x = v.initialization() + 0.05 * np.random.default_rng(3).standard_normal(v.dim_n * 64 * 65)
            cache[tag] = (v, _fields(v), x)
        else:                                       # "l96d4", "l96d5": an oracle problem on a bare context
            q, x = make_problem("L96", int(tag[4:]), 41, method="euler")
            cache[tag] = (None, q, x)
    return cache[tag]


SEED_W = 77


def _given(q):
    return np.reshape(np.asarray(q.m0, dtype=float), q.dim_d) + 0.1


def _reference(cache, tag, start):
    key = (tag, start)
    if key not in cache:
        _, q, x = _case(cache, tag)
        cache[key] = path_weights_numpy(q, x, _given(q) if start == "given" else None, N_MAX, SEED_W)
    return cache[key]


def _weights(v, q, x, n_paths, seed, x0):
    """(init, path, obs) from the device: VarGP.importance_weights, or the bare context and the host-side init term"""
    if v is not None:
        w = v.importance_weights(n_paths, seed, x=x, x0=x0)
        assert w.paths is None
        return w.init, w.path, w.obs
    ctx = gpu_context(q)
    paths, logw, start = ctx.sample_paths_weighted(n_paths, seed, x=x, x0=x0, paths=False)
    ctx.close()
    assert paths is None
    init = np.zeros(n_paths) if x0 is not None else init_term(start[0], q.mu0, q.tau0, q.m0, q.s0)
    return init, logw[0, :, 0], logw[0, :, 1]


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("n_paths", [1, 17, 65])
@pytest.mark.parametrize("tag", TAGS)
def test_against_numpy(cases, tag, n_paths, start):
    v, q, x = _case(cases, tag)
    want = _reference(cases, tag, start)
    scale = want[3][:n_paths]
    got = _weights(v, q, x, n_paths, SEED_W, _given(q) if start == "given" else None)
    worst = {}
    for name, g, w in zip(("init", "path", "obs"), got, want[:3]):
        assert g.shape == (n_paths,) and np.all(np.isfinite(g)), name
        worst[name] = _excess(g, w[:n_paths], scale)
    print(tag, n_paths, start, "worst |got - want| / (1 + scale):", worst, " scale up to", float(scale.max()))
    assert worst["path"] <= TOL and worst["obs"] <= TOL and worst["init"] <= TOL
    assert start == "drawn" or np.all(got[0] == 0.0)


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p", "l96d40_rk4_p", "l96d64"])
def test_paths_and_starts(cases, tag):
    """the paths are those of sample_paths with the same arguments; start holds their k = 0 points; paths=False changes no weight"""
    v, q, x = _case(cases, tag)
    ctx = v._context()
    for stride, x0 in [(1, None), (4, _given(q))]:
        plain = ctx.sample_paths("posterior", 17, 5, stride=stride, x=x, x0=x0)
        paths, logw, start = ctx.sample_paths_weighted(17, 5, stride=stride, x=x, x0=x0)
        none, logw_only, start_only = ctx.sample_paths_weighted(17, 5, stride=stride, x=x, x0=x0, paths=False)
        print(tag, "stride", stride, "paths bit-equal to sample_paths:", bool(np.array_equal(paths, plain)))
        assert paths.shape == plain.shape and rel_err(paths, plain) <= TOL
        assert np.array_equal(start, paths[:, :, 0]) and np.array_equal(start_only, start)
        assert none is None and np.array_equal(logw_only, logw)
        assert logw.shape == (1, 17, 2) and start.shape == (1, 17, q.dim_d)
    w = v.importance_weights(17, 5, x=x, stride=4)
    kept = np.asarray(v.sample_paths(17, 5, stride=4, x=x))
    assert w.paths.shape == kept.shape and rel_err(w.paths, kept) <= TOL


@pytest.mark.parametrize("tag", ["l63_euler_p", "l96d12_euler_p"])
def test_independent_form_from_the_devices_own_paths(cases, tag):
    v, q, x = _case(cases, tag)
    scale = _reference(cases, tag, "drawn")[3][:17]
    paths, logw, _ = v._context().sample_paths_weighted(17, SEED_W, x=x)
    worst = _excess(logw[0, :, 0], independent_form(q, x, paths[0]), scale)
    print(tag, "worst |path term - independent form| / (1 + scale) =", worst)
    assert worst <= TOL


def test_ou_with_the_models_own_drift():
    z = load_golden("ou_euler")
    v = problem_from_golden(z)["vgp"]
    x = np.concatenate((np.full(v.dim_n, float(v.model.theta)), np.zeros(v.dim_n)))
    w = v.importance_weights(65, 3, x=x)
    v.invalidate()
    print("OU, A_t = theta, b_t = 0: max |path term| =", float(np.max(np.abs(w.path))))
    assert np.max(np.abs(w.path)) <= 1e-12 and np.all(np.isfinite(w.obs))


@pytest.mark.parametrize("obs_at", [(0, 7, 20), (5, 40), (10, 11, 12), (0, 1, 39, 40)], ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 applies to x_0, one at Np - 1 to the last state; adjacent indices"""
    q, x = make_problem(model, d, 41, method="euler", obs_at=list(obs_at))
    if model == "L63":          # (make_problem's b_t aims at 8 m0: a drift for Lorenz-96; keep the Lorenz-63 chain near its data)
        x = np.concatenate((x[:41 * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(41, axis=0).ravel()))
    ctx = gpu_context(q)
    for x0 in (None, _given(q)):
        _, logw, start = ctx.sample_paths_weighted(17, 9, x=x, x0=x0, paths=False)
        init, path, obs, scale = path_weights_numpy(q, x, x0, 17, 9)
        worst = max(_excess(logw[0, :, 0], path, scale), _excess(logw[0, :, 1], obs, scale))
        print(model, obs_at, "given" if x0 is not None else "drawn", "worst", worst)
        assert worst <= TOL
    ctx.close()


@pytest.mark.parametrize("model,d,n_paths", [("L96", 12, 17), ("L63", 3, 40)])
def test_batch_with_own_rows(model, d, n_paths):
    """B = 3: own observation count, dense R and H, own times and values, own theta, own isotropic Sigma, own prior moments.  D <= 4 with 40
    paths per problem: the lanes of a wave belong to different problems."""
    nb, n = 3, 41
    rng = np.random.default_rng(11)
    times = [np.array([0, 6, 13, 27, 40]), np.array([3, 4, 30, 39]), np.array([9, 21, 22])]
    probs, xs = [], []
    for k in range(nb):
        q, x = make_problem(model, d, n, method="euler", seed=20 + k, obs_at=list(times[k]))
        if model == "L63":
            x = np.concatenate((x[:n * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(n, axis=0).ravel()))
        theta = np.asarray(q.theta, dtype=float) * (1.0 + 0.05 * k)
        q = dataclasses.replace(q, theta=theta if theta.ndim else float(theta), sigma=(3.0 + 0.4 * k) * np.eye(d),
                                s0=np.asarray(q.s0) * (1.0 + 0.1 * k), obs_noise=spd(rng, d, 1.0 + 0.2 * k, 0.2),
                                obs_h=np.eye(d) + 0.1 * rng.standard_normal((d, d)))
        probs.append(q)
        xs.append(x)
    xs = np.stack(xs)
    m = max(t.size for t in times)
    obs_t, obs_y = np.full((nb, m), -1, dtype=np.int64), np.full((nb, m, d), np.nan)
    for k, q in enumerate(probs):
        obs_t[k, :times[k].size], obs_y[k, :times[k].size] = times[k], q.obs_y
    p0 = probs[0]
    ctx = va.Context(model, "euler", d, n, p0.dt, sigma=p0.sigma, theta=np.atleast_1d(p0.theta), m0=p0.m0, s0=p0.s0, obs_t=p0.obs_t,
                     obs_y=p0.obs_y, obs_noise=p0.obs_noise, obs_h=p0.obs_h, batch=nb)
    ctx.set_problem_obs_model(n_obs=[t.size for t in times], obs_noise=np.stack([q.obs_noise for q in probs]),
                              obs_h=np.stack([q.obs_h for q in probs]))
    ctx.set_problem_data(obs_t=obs_t, obs_y=obs_y, m0=np.stack([q.m0 for q in probs]), s0=np.stack([q.s0 for q in probs]))
    ctx.set_problem_params(theta=np.stack([np.atleast_1d(q.theta) for q in probs]), sigma=np.stack([q.sigma for q in probs]))
    x0 = np.stack([_given(q) for q in probs])
    drawn = ctx.sample_paths_weighted(n_paths, 13, x=xs, paths=False)
    ctx.free_energy(xs)
    cached = ctx.sample_paths_weighted(n_paths, 13, paths=False)               # x=None: the x of that evaluation
    given = ctx.sample_paths_weighted(n_paths, 13, x=xs, x0=x0, paths=False)
    ctx.close()
    assert np.array_equal(drawn[1], cached[1]) and np.array_equal(drawn[2], cached[2])
    for k, q in enumerate(probs):
        for (_, logw, start), s0 in ((drawn, None), (given, x0[k])):
            init, path, obs, scale = path_weights_numpy(q, xs[k], s0, n_paths, 13, index=k)
            worst = max(_excess(logw[k, :, 0], path, scale), _excess(logw[k, :, 1], obs, scale))
            print(model, "problem", k, "given" if s0 is not None else "drawn", "worst", worst)
            assert worst <= TOL
            if s0 is None:
                assert _excess(init_term(start[k], q.mu0, q.tau0, q.m0, q.s0), init, scale) <= TOL
            else:
                assert np.array_equal(start[k], np.tile(s0, (n_paths, 1)))


def test_problem_batch_records():
    """ProblemBatch.importance_weights: one record per member, each with its own prior, against the numpy restatement of index p"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.importance_weights(17, 8, x=x)
    kept = pb.importance_weights(17, 8, x=x, stride=10)
    pb.close()
    assert len(recs) == len(kept) == 3
    for k, p in enumerate(ps):
        init, path, obs, scale = path_weights_numpy(_fields(p["vgp"]), x[k], None, 17, 8, index=k)
        for name, g, w in (("init", recs[k].init, init), ("path", recs[k].path, path), ("obs", recs[k].obs, obs)):
            assert _excess(g, w, scale) <= TOL, (k, name)
        assert recs[k].paths is None and kept[k].paths.shape == (17, 6, 12) and np.array_equal(kept[k].log_w, recs[k].log_w)
        assert np.isfinite(recs[k].log_evidence()) and 1.0 <= recs[k].ess() <= 17.0


CACHE_CASES = [("L63", "rk4", None, 1.0, 65), ("L96", "rk4", 40, 0.5, 65), ("L96", "rk4", 12, 0.5, 1)]


@pytest.mark.parametrize("case", CACHE_CASES, ids=lambda c: f"{c[0]}{c[2] or ''}-B{c[4]}")
def test_the_cache_is_not_touched(case):
    """gradient(None), fetch of mt / st / lamt and theta_gradient() behind sample_paths_weighted(x=None) are bit for bit what they are
    without the call (the orders of test_sample_paths.test_the_cache_is_not_touched: recording changes the state by itself)."""
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.sample_paths_weighted(3, 4, stride=10)[1] for step in order]
        ctx.close()
        return out

    a1, logw, a2 = run(["record", "sample", "record"])
    b1, b2 = run(["record", "record"])
    logw_c, c1 = run(["sample", "record"])
    assert np.array_equal(logw, logw_c) and np.all(np.isfinite(logw))
    for k, what in enumerate(("gradient", "mt", "st", "lamt", "theta_gradient")):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), what
        assert np.array_equal(a2[k], b2[k]), what
    k = nb - 1
    _, path, obs, scale = path_weights_numpy(probs[k], xs[k], None, 3, 4, index=k)
    assert max(_excess(logw[k, :, 0], path, scale), _excess(logw[k, :, 1], obs, scale)) <= TOL


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    usable = lambda: ctx.sample_paths_weighted(2, 1, stride=25, x=xs)[1]       # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.sample_paths_weighted(2, 1)
    ref = usable()
    with pytest.raises(ValueError):
        ctx.sample_paths_weighted(0, 1, x=xs)
    with pytest.raises(ValueError):
        ctx.sample_paths_weighted(2, 1, stride=0, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.sample_paths_weighted(bad, 1, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.sample_paths_weighted(2, 1, stride=bad, x=xs)
    assert np.array_equal(usable(), ref)
    xx = np.ascontiguousarray(xs)                                               # a null logw, through the C ABI itself
    rc = ctx._lib.vgpa_sample_paths_weighted(ctx._h, xx.ctypes.data, None, 2, 1, 1, None, None, None)
    assert rc == -1
    assert np.array_equal(usable(), ref)
    # a dense Sigma in force
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    assert ctx.sample_paths("posterior", 2, 1, stride=25, x=xs).shape == (3, 2, 3, 12)      # (the sampler itself takes it)
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert np.array_equal(usable(), ref)
    # an S0 row that is not positive definite: refused for a drawn start, not needed for a given one
    s0 = np.stack([np.reshape(q.s0, (12, 12)) for q in probs])
    s0[2, 5, 5] = -0.2
    ctx.set_problem_data(obs_y=np.stack([np.reshape(q.obs_y, (-1, 12)) for q in probs]), m0=np.stack([q.m0 for q in probs]), s0=s0)
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        usable()
    assert ctx.sample_paths_weighted(2, 1, stride=25, x=xs, x0=np.zeros((3, 12)))[1].shape == (3, 2, 2)
    ctx.close()
    # no model: ValueError; a model without prior moments and observations (ODE-only): RuntimeError
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.sample_paths_weighted(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.sample_paths_weighted(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    # D > 64
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.sample_paths_weighted(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()
