"""
Sample paths of the posterior process and of the model SDE on the GPU (vgpa_sample_paths).

Reference: the numpy restatement of the generator and of the Euler-Maruyama recursion in test_sample_paths_cpu.py, evaluated with each
problem's own rows.  Tolerance: the suite's TOL = 1e-9 (max-norm relative, conftest.rel_err) unless a test says otherwise.

(Lorenz-96 at D = 5 comes from test_gpu_edge_cases.make_problem, not from build_problem: the host class Lorenz96 refuses D < 10, as the
reference's does, while the library's kernels start at D = 4.  Same sizes, same checks.)
"""
import dataclasses
import types

import numpy as np
import pytest

import vgpa_amd as va
from conftest import load_golden, rel_err
from helpers import SEED, build_problem, make_model, problem_from_golden
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_path_weights_cpu import FIXTURES, TAGS
from test_sample_paths_cpu import em_moments, n_keep, normals, sample_paths_numpy

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def cases():
    """the posterior problems, built once per tag and shared by the tests of this module; their contexts are closed behind the last one"""
    cache = {}
    yield cache
    for v, _, _ in cache.values():
        if v is not None:
            v.invalidate()


def _fields(vgp):
    """what the numpy recursion reads of one VarGP: its inputs NOW"""
    inp = vgp._inputs()
    return types.SimpleNamespace(model=vgp.model._model_id, dim_d=vgp.dim_d, n_pts=vgp.dim_n, dt=float(vgp.fwd_ode.dt),
                                 theta=inp["theta"] if inp["theta"].size > 1 else float(inp["theta"][0]), sigma=inp["sigma"],
                                 m0=inp["m0"], s0=inp["s0"])


def _posterior_case(cache, tag):
    """(VarGP, fields for the numpy recursion, x) -- built once per tag"""
    if tag not in cache:
        if tag in FIXTURES:
            z = load_golden(tag)
            v = problem_from_golden(z)["vgp"]
            cache[tag] = (v, _fields(v), np.asarray(z["x"], dtype=float))
        elif tag == "l96d64":
            p = build_problem("L96", "euler", 0.5, dim_d=64)
            v = p["vgp"]
            x = v.initialization() + 0.05 * np.random.default_rng(3).standard_normal(v.dim_n * 64 * 65)
            cache[tag] = (v, _fields(v), x)
        elif tag == "none_d2":                      # no stochastic model: the one way to D = 2, and to the posterior kind alone
            rng = np.random.default_rng(5)
            q = types.SimpleNamespace(model="NONE", dim_d=2, n_pts=41, dt=0.01, theta=0.0, sigma=np.diag(3.0 + rng.random(2)),
                                      m0=1.0 + rng.standard_normal(2), s0=np.array([[0.2, 0.05], [0.05, 0.3]]))
            x = np.concatenate(((2.0 * np.eye(2) + 0.05 * rng.standard_normal((41, 2, 2))).ravel(), rng.standard_normal(41 * 2)))
            cache[tag] = (None, q, x)
        else:                                       # "l96d4", "l96d5": an oracle problem on a bare context
            q, x = make_problem("L96", int(tag[4:]), 41, method="euler")
            cache[tag] = (None, q, x)
    return cache[tag]


def _draw(v, q, x, n_paths, seed, stride, x0):
    if v is not None:
        return np.asarray(v.sample_paths(n_paths, seed, stride=stride, x=x, x0=x0)).reshape(n_paths, -1, q.dim_d)
    ctx = gpu_context(q) if q.model != "NONE" else va.Context("NONE", "euler", q.dim_d, q.n_pts, q.dt, sigma=q.sigma, m0=q.m0, s0=q.s0)
    out = ctx.sample_paths("posterior", n_paths, seed, stride=stride, x=x, x0=x0)[0]
    ctx.close()
    return out


def test_generator_on_the_device():
    """x = 0 and x0 = 0 with Sigma = I: (x_k - x_{k-1}) / sqrt(dt) are the normals themselves.  1e-12 absolute: |xi| <= 8.65 by
    construction, the device log / sincos and the differencing are at the 1e-15 level.  Odd D: the dropped half pair; B = 2 and three paths:
    the counter words."""
    d, n, nb, n_paths, seed, dt = 17, 21, 2, 3, 0x1234567890ABCDEF, 0.01
    ctx = va.Context("L96", "euler", d, n, dt, sigma=np.eye(d), theta=[8.0], batch=nb)
    got = ctx.sample_paths("posterior", n_paths, seed, x=np.zeros((nb, n * d * (d + 1))), x0=np.zeros((nb, d)))
    ctx.close()
    assert got.shape == (nb, n_paths, n, d) and np.all(got[:, :, 0] == 0.0)
    xi = np.diff(got, axis=2) / np.sqrt(dt)
    worst = 0.0
    for p in range(nb):
        want = normals(seed, np.arange(1, n)[None, :], np.arange(n_paths)[:, None], p, d)
        worst = float(np.maximum(worst, np.max(np.abs(xi[p] - want))))
    print("generator: max |xi_device - xi_numpy| =", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("n_paths", [1, 16, 17, 65])
@pytest.mark.parametrize("tag", TAGS + ["none_d2"])
def test_posterior_paths_against_numpy(cases, tag, n_paths):
    v, q, x = _posterior_case(cases, tag)
    d, n = q.dim_d, q.n_pts
    given = np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1
    worst = 0.0
    for stride, x0 in [(1, None), (1, given), (4, None), (4, given), (n + 3, None)]:
        got = _draw(v, q, x, n_paths, 99 + stride, stride, x0)
        want = sample_paths_numpy(q, "posterior", x, x0, n_paths, stride, 99 + stride)
        assert got.shape == want.shape == (n_paths, n_keep(n, stride), d) and np.all(np.isfinite(got))
        worst = float(np.maximum(worst, rel_err(got, want)))       # (np.maximum: a NaN stays a NaN)
    print(tag, n_paths, "worst rel err", worst)
    assert worst <= TOL


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "l96d40_rk4_p"])
def test_prefix_property(cases, tag):
    v, q, x = _posterior_case(cases, tag)
    a = np.asarray(v.sample_paths(65, 5, stride=2, x=x))
    b = np.asarray(v.sample_paths(17, 5, stride=2, x=x))
    assert np.array_equal(a[:17], b)
    assert not np.array_equal(a[17:34], b)


def test_problems_of_a_batch_draw_their_own_numbers():
    """three members with the SAME data: problem p differs from problem 0 through the counter word alone, and equals the numpy recursion
    of index p"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=SEED) for _ in range(3)]
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    got = pb.sample_paths(17, 8, stride=4, x=x)
    pb.close()
    assert got.shape == (3, 17, n_keep(ps[0]["vgp"].dim_n, 4), 12)
    q = _fields(ps[0]["vgp"])
    for p in range(3):
        assert rel_err(got[p], sample_paths_numpy(q, "posterior", x[p], None, 17, 4, 8, index=p)) <= TOL, p
        assert p == 0 or not np.array_equal(got[p], got[0])


def _own_batch(name, d, nb, form):
    """nb VarGPs with own data, own prior moments and (form != None) own theta / Sigma: iso, diag or dense"""
    ps = [build_problem(name, "euler", 0.5, dim_d=d, seed=SEED + k) for k in range(nb)]
    for k, p in enumerate(ps):
        v, m = p["vgp"], p["model"]
        v.output["s0"] = np.asarray(v.output["s0"], dtype=float) * (1.0 + 0.05 * k)
        if form is None:
            continue
        m.theta = np.asarray(m.theta, dtype=float) * (1.0 + 0.05 * k) if name == "L63" else float(m.theta) * (1.0 + 0.05 * k)
        if m.single_dim:
            m.sigma = float(m.sigma) * (1.0 + 0.1 * k)
        else:
            dd = v.dim_d
            s, rho = float(np.mean(np.diag(m.sigma))), 0.1 * (1 + k)
            m.sigma = {"iso": s * (1.0 + 0.1 * k) * np.eye(dd), "diag": np.diag(s * (1.0 + 0.1 * ((np.arange(dd) + k) % 3))),
                       "dense": s * (1.0 + 0.05 * k) * ((1.0 - rho) * np.eye(dd) + rho * np.ones((dd, dd)))}[form]
    return ps


@pytest.mark.parametrize("name,d,form", [("L96", 12, None), ("L96", 12, "dense"), ("L96", 12, "diag"), ("L96", 40, "iso"), ("L63", None, "dense"),
                                         ("OU", None, "iso"), ("DW", None, "iso")], ids=lambda v: str(v))
def test_per_problem_inputs(name, d, form):
    nb = 3
    ps = _own_batch(name, d, nb, form)
    pb = va.ProblemBatch([p["vgp"] for p in ps], own_parameters=form is not None)
    x = pb.initialization()
    post = pb.sample_paths(17, 21, stride=3, x=x)                       # drawn start: own m0 / S0
    pb.free_energy(x)
    post_cached = pb.sample_paths(17, 21, stride=3)                     # x=None: the x of that evaluation
    model = pb.sample_paths(17, 22, stride=3, kind="model")
    pb.close()
    assert np.array_equal(post, post_cached)
    for k, p in enumerate(ps):
        q = _fields(p["vgp"])
        assert rel_err(post[k], sample_paths_numpy(q, "posterior", x[k], None, 17, 3, 21, index=k)) <= TOL, k
        assert rel_err(model[k], sample_paths_numpy(q, "model", None, None, 17, 3, 22, index=k)) <= TOL, k


# (model, method, D, tf, B): Np <= 61
MODEL_KIND = [("OU", "euler", None, 0.5, 3), ("OU", "euler", None, 0.5, 600), ("DW", "euler", None, 0.5, 3), ("DW", "euler", None, 0.5, 600),
              ("L63", "euler", None, 0.6, 3), ("L63", "euler", None, 0.6, 600), ("L96", "euler", 12, 0.5, 3), ("L96", "euler", 40, 0.5, 3)]


@pytest.mark.parametrize("case", MODEL_KIND, ids=lambda c: f"{c[0]}{c[2] or ''}-B{c[4]}")
def test_model_kind(case):
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    # (_datasets shifts m0 by 0.01 k: at k = 599 an Euler-Maruyama step of the double well is past its stability bound.  Own m0 within 0.1.)
    probs = [dataclasses.replace(q, m0=q.m0 - 0.01 * k + 0.002 * (k % 50)) for k, q in enumerate(probs)]
    ctx = _context(base, probs, nb, 0, obs_t=False)
    dd = probs[0].dim_d
    x0 = np.stack([np.reshape(np.asarray(q.m0, dtype=float), dd) - 0.05 * (k % 5) for k, q in enumerate(probs)])
    drawn = ctx.sample_paths("model", 5, 31, stride=3)
    given = ctx.sample_paths("model", 5, 31, stride=1, x0=x0)
    ctx.close()
    assert drawn.shape == (nb, 5, n_keep(probs[0].n_pts, 3), dd) and given.shape == (nb, 5, probs[0].n_pts, dd)
    assert np.all(np.isfinite(drawn)) and np.all(np.isfinite(given))
    worst = 0.0
    for k in sorted({0, 1, 2, nb // 2, nb - 1}):
        worst = float(np.max([worst, rel_err(drawn[k], sample_paths_numpy(probs[k], "model", None, None, 5, 3, 31, index=k)),
                              rel_err(given[k], sample_paths_numpy(probs[k], "model", None, x0[k], 5, 1, 31, index=k))]))
    print(case, "worst rel err", worst)
    assert worst <= TOL


@pytest.mark.parametrize("name,d,tf", [("OU", None, 0.5), ("DW", None, 0.5), ("L63", None, 0.6), ("L96", 12, 0.5), ("L96", 40, 0.25)])
def test_sample_trajectories(name, d, tf):
    model = make_model(name, d)
    dd = 1 if model.single_dim else model.dim_d
    x0 = 0.5 + 0.1 * np.arange(dd) if name != "L96" else 8.0 + 0.1 * np.arange(dd)
    tk, paths = model.sample_trajectories(x0, 7, 0.0, tf, 0.01, seed=12, stride=2)
    full = np.arange(0.0, tf + 0.01, 0.01)
    assert np.array_equal(tk, full[::2])
    q = types.SimpleNamespace(model=name, dim_d=dd, n_pts=full.size, dt=0.01, theta=model.theta, sigma=model.sigma, m0=None, s0=None)
    want = sample_paths_numpy(q, "model", None, x0, 7, 2, 12)
    assert paths.shape == ((7, tk.size) if model.single_dim else (7, tk.size, dd))
    assert rel_err(np.reshape(paths, want.shape), want) <= TOL
    assert model.tk is None and model.xt is None          # make_trajectory's members are not involved


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p"])
def test_moments(cases, tag):
    """Sample mean and unbiased sample variance of 4096 paths against the moments of the Euler-Maruyama chain itself (not fetch("mt") /
    fetch("st"): the forward ODE's S_t lacks the dt^2 A S A^T term).  4.5 standard errors at every component and grid point; with this
    seed the numpy restatement alone reaches 2.74 (means) and 2.90 (variances)."""
    v, q, x = _posterior_case(cases, tag)
    k_paths = 4096
    got = np.asarray(v.sample_paths(k_paths, 20261018, x=x)).reshape(k_paths, q.n_pts, q.dim_d)
    m, s = em_moments(q, x)
    var = np.diagonal(s, axis1=1, axis2=2)
    zm = np.abs(got.mean(axis=0) - m) / np.sqrt(var / k_paths)
    zv = np.abs(got.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / (k_paths - 1)))
    print(tag, "worst mean z", zm.max(), "worst variance z", zv.max())
    assert zm.max() <= 4.5 and zv.max() <= 4.5


CACHE_CASES = [("L63", "rk4", None, 1.0, 600), ("L96", "rk4", 40, 0.5, 65), ("L96", "rk4", 12, 0.5, 1)]


@pytest.mark.parametrize("case", CACHE_CASES, ids=lambda c: f"{c[0]}{c[2] or ''}-B{c[4]}")
def test_the_cache_is_not_touched(case):
    """gradient(None), fetch of mt / st / lamt and theta_gradient() behind sample_paths(x=None) are bit for bit what they are without the
    call.  Recording changes the state by itself (on the lane-pass context fetch("lamt") materialises the per-grid-point terms and the next
    gradient(None) is assembled from them), so a second recording is compared with the second recording of a context that never drew:
        A: free_energy, record, sample_paths, record      B: free_energy, record, record      C: free_energy, sample_paths, record"""
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.sample_paths("posterior", 3, 4, stride=10) for step in order]
        ctx.close()
        return out

    a1, paths, a2 = run(["record", "sample", "record"])
    b1, b2 = run(["record", "record"])
    paths_c, c1 = run(["sample", "record"])
    assert np.array_equal(paths, paths_c)
    for k, what in enumerate(("gradient", "mt", "st", "lamt", "theta_gradient")):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), what
        assert np.array_equal(a2[k], b2[k]), what
    k = nb - 1
    assert rel_err(paths[k], sample_paths_numpy(probs[k], "posterior", xs[k], None, 3, 10, 4, index=k)) <= TOL


def test_errors():
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    usable = lambda: ctx.sample_paths("posterior", 2, 1, stride=25, x=xs)       # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.sample_paths("posterior", 2, 1)
    ref = usable()
    with pytest.raises(RuntimeError, match="cached"):                           # an x of its own drops what was cached
        ctx.free_energy(xs)
        ctx.sample_paths("posterior", 2, 1, x=xs)
        ctx.gradient(None)
    with pytest.raises(ValueError):
        ctx.sample_paths("model", 2, 1, x=xs)
    with pytest.raises(ValueError):
        ctx.sample_paths("posterior", 0, 1, x=xs)
    with pytest.raises(ValueError):
        ctx.sample_paths("posterior", 2, 1, stride=0, x=xs)
    with pytest.raises(ValueError):
        ctx.sample_paths("neither", 2, 1, x=xs)
    for bad in (2 ** 31, 2 ** 32 + 1, -2 ** 31 - 1):      # (would wrap on its way into the int32 of the C ABI)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.sample_paths("posterior", bad, 1, x=xs)
        with pytest.raises(ValueError, match="32 bits"):
            ctx.sample_paths("posterior", 2, 1, stride=bad, x=xs)
    assert np.array_equal(usable(), ref)
    # a per-problem Sigma / S0 that is not positive definite
    bad = np.stack([np.reshape(q.sigma, (12, 12)) for q in probs])
    bad[1, 3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):             # (refused by the setter: a bad Sigma is never in force, so the sampler cannot meet one;
        ctx.set_problem_params(sigma=bad)                  #  the previous rows stay, and the draws are what they were)
    assert np.array_equal(usable(), ref)
    s0 = np.stack([np.reshape(q.s0, (12, 12)) for q in probs])
    s0[2, 5, 5] = -0.2
    ctx.set_problem_data(obs_y=np.stack([np.reshape(q.obs_y, (-1, 12)) for q in probs]), m0=np.stack([q.m0 for q in probs]), s0=s0)
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        usable()
    assert ctx.sample_paths("posterior", 2, 1, stride=25, x=xs, x0=np.zeros((3, 12))).shape == (3, 2, 3, 12)
    ctx.close()
    # no model, no prior moments
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    x = np.zeros((2, 10 * 12))
    with pytest.raises(ValueError):
        ode.sample_paths("model", 2, 1, x0=np.zeros((2, 3)))
    with pytest.raises(RuntimeError):
        ode.sample_paths("posterior", 2, 1, x=x)                                # no m0 / s0 to draw the start from
    assert ode.sample_paths("posterior", 2, 1, x=x, x0=np.ones((2, 3))).shape == (2, 2, 10, 3)
    ode.close()
    # D > 64
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.sample_paths("posterior", 2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()
