"""
Importance weights of sampled posterior paths (vgpa_sample_paths_weighted): the numpy restatement, its checks against an independent form
and against the energies of the fixtures, the PathWeights record and the host-side surface.

The restatement is the reference of tests/test_path_weights.py.  It walks the recursion of test_sample_paths_cpu.sample_paths_numpy (the
same normals, the same model drift) and sums, per path,
    path = sum_k [ -d^T Sigma^-1 eta_k - dt d^T Sigma^-1 d / 2 ],  d = g - f at x_{k-1},  eta_k = chol(Sigma dt) xi_k
    obs  = sum_n [ -(y_n - x_{t_n})^T Q (y_n - x_{t_n}) / 2 ] - M (D log 2 pi + log det R) / 2,  Q = H R^-1 H^T
    init = log N(x_0; mu0, tau0) - log N(x_0; m0, S0)   (0 for a given start)
with scale = sum_k |increment_k| of the path term, the size rounding errors are measured against.
"""
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.weights import PathWeights, gauss_logpdf, init_term
from conftest import ROOT, load_golden
from oracle import vgpa_oracle as vo
from test_sample_paths_cpu import em_noise, em_step, model_drift, sample_paths_numpy, start_cloud

FIXTURES = ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p", "l96d40_rk4_p"]
# the tags of the sampler tests: the fixtures, "l96d<D>" = make_problem("L96", D, 41, method="euler") on a bare context (D = 4: the widest
# one-lane-per-path kernel, D = 5: the narrowest matrix-core one) and "l96d64", a built problem at the widest
TAGS = FIXTURES + ["l96d4", "l96d5", "l96d64"]


def _split(problem, x):
    d, n = int(problem.dim_d), int(problem.n_pts)
    x = np.asarray(x, dtype=float)
    return x[:n * d * d].reshape(n, d, d), x[n * d * d:].reshape(n, d)


def _sigma_diag(problem):
    d = int(problem.dim_d)
    sigma = np.reshape(np.asarray(problem.sigma, dtype=float), (d, d))
    assert np.array_equal(sigma, np.diag(sigma.diagonal())), "the weights are defined for a diagonal Sigma"
    return sigma


def obs_model(problem):
    """(obs_t (M,), obs_y (M, D), Q (D, D), the additive constant M (D log 2 pi + log det R) / 2) of one problem"""
    d = int(problem.dim_d)
    obs_t = np.asarray(problem.obs_t, dtype=np.int64).ravel()
    obs_y = np.asarray(problem.obs_y, dtype=float).reshape(obs_t.size, d)
    r = np.reshape(np.asarray(problem.obs_noise, dtype=float), (d, d))
    h = getattr(problem, "obs_h", None)
    h = np.eye(d) if h is None or d == 1 else np.reshape(np.asarray(h, dtype=float), (d, d))
    q = h @ np.linalg.inv(r) @ h.T
    return obs_t, obs_y, q, 0.5 * obs_t.size * (d * np.log(2.0 * np.pi) + np.linalg.slogdet(r)[1])


def start_term(problem, state, x0):
    """(n,): init of the module's docstring for the start `state` of start_cloud -- 0 for a given start"""
    if x0 is not None:
        return np.zeros(state.shape[0])
    return init_term(state, problem.mu0, problem.tau0, problem.m0, problem.s0)


def path_increment(dd, eta, isg, dt):
    """(n,): one step's term of `path` for d = dd (n, D), eta (n, D) and the diagonal isg of Sigma^-1"""
    return -np.sum(dd * isg * eta, axis=1) - 0.5 * dt * np.sum(dd * isg * dd, axis=1)


def observation_term(y, state, q):
    """(n,): one observation's term of `obs` (without the constant) for the states (n, D)"""
    r = y[None, :] - state
    return -0.5 * np.einsum("pi,ij,pj->p", r, q, r)


def path_weights_numpy(problem, x, x0, n_paths, seed, index=0):
    """(init, path, obs, scale), each (n_paths,), of the paths sample_paths_numpy(problem, "posterior", x, x0, n_paths, 1, seed, index) draws"""
    d, n, dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
    sigma = _sigma_diag(problem)
    isg, fac = 1.0 / sigma.diagonal(), np.linalg.cholesky(sigma * dt)
    lin_a, off_b = _split(problem, x)
    theta = np.asarray(problem.theta, dtype=float)
    obs_t, obs_y, q, const = obs_model(problem)
    at = {int(t): k for k, t in enumerate(obs_t)}
    paths = np.arange(n_paths)
    state = start_cloud(problem, x0, seed, paths, index)
    init = start_term(problem, state, x0)
    path, scale, obs = np.zeros(n_paths), np.zeros(n_paths), np.full(n_paths, -const)

    def observe(k):
        if k in at:
            obs[:] += observation_term(obs_y[at[k]], state, q)

    observe(0)
    for k in range(1, n):
        g = -(state @ lin_a[k - 1].T) + off_b[k - 1]
        dd = g - model_drift(problem.model, theta, state)
        eta = em_noise(seed, k, paths, index, fac)
        inc = path_increment(dd, eta, isg, dt)
        path += inc
        scale += np.abs(inc)
        state = em_step(state, dt, g, eta)
        observe(k)
    return init, path, obs, scale


def independent_form(problem, x, stored):
    """sum_k [log N(x_k; x_{k-1} + f dt, Sigma dt) - log N(x_k; x_{k-1} + g dt, Sigma dt)] from stored stride-1 paths (n_paths, Np, D)"""
    d, n, dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
    cov = _sigma_diag(problem) * dt
    lin_a, off_b = _split(problem, x)
    theta = np.asarray(problem.theta, dtype=float)
    total = np.zeros(stored.shape[0])
    for k in range(1, n):
        prev, new = stored[:, k - 1], stored[:, k]
        g = -(prev @ lin_a[k - 1].T) + off_b[k - 1]
        f = model_drift(problem.model, theta, prev)
        total += gauss_logpdf(new - (prev + dt * f), np.zeros(d), cov) - gauss_logpdf(new - (prev + dt * g), np.zeros(d), cov)
    return total


def _fixture(tag):
    z = load_golden(tag)
    return z, vo.Problem.from_fixture(z), np.asarray(z["x"], dtype=float)


@pytest.mark.parametrize("tag", FIXTURES)
def test_sum_against_the_independent_form(tag):
    _, p, x = _fixture(tag)
    worst = 0.0
    for x0 in (None, np.reshape(np.asarray(p.m0, dtype=float), p.dim_d) + 0.1):
        _, path, _, scale = path_weights_numpy(p, x, x0, 9, 5)
        stored = sample_paths_numpy(p, "posterior", x, x0, 9, 1, 5)
        err = np.abs(path - independent_form(p, x, stored)) / (1.0 + scale)
        worst = max(worst, float(err.max()))
        assert np.all(np.isfinite(path)) and np.all(scale > 0.0)
    print(tag, "worst |sum - independent| / (1 + scale) =", worst)
    assert worst <= 1e-12


def test_ou_with_the_models_own_drift_has_no_path_term():
    _, p, _ = _fixture("ou_euler")
    x = np.concatenate((np.full(p.n_pts, float(p.theta)), np.zeros(p.n_pts)))
    _, path, obs, scale = path_weights_numpy(p, x, None, 33, 3)
    assert np.all(path == 0.0) and np.all(scale == 0.0) and np.all(np.isfinite(obs))


def test_ou_sanity_numbers():
    """4096 paths, seed 7 (deterministic draws).  E[exp(path)] = 1 exactly; -E_sde and -E_obs are the expectations of the path and observation
    terms under the moments the fixture's energies were computed from.  The bounds are 4-5 standard errors of the measured values."""
    z, p, x = _fixture("ou_euler")
    _, path, obs, _ = path_weights_numpy(p, x, None, 4096, 7)
    lme = float(np.log(np.mean(np.exp(path))))
    print("log mean exp(path) =", lme, " mean(path) =", path.mean(), "+-", path.std() / 64.0, " -E_sde =", -float(z["Esde"]),
          " mean(obs) =", obs.mean(), "+-", obs.std() / 64.0, " -E_obs =", -float(z["Eobs"]))
    assert abs(lme) <= 0.05
    assert abs(path.mean() + float(z["Esde"])) <= 0.05
    assert abs(obs.mean() + float(z["Eobs"])) <= 0.8


def test_init_term():
    _, p, x = _fixture("l63_euler_p")
    init, _, _, _ = path_weights_numpy(p, x, None, 5, 2)
    start = sample_paths_numpy(p, "posterior", x, None, 5, p.n_pts, 2)[:, 0]
    d = p.dim_d

    def logn(v, mean, cov):
        zc = v - mean
        return -0.5 * zc @ np.linalg.solve(cov, zc) - 0.5 * np.linalg.slogdet(cov)[1] - 0.5 * d * np.log(2.0 * np.pi)

    want = [logn(s, np.asarray(p.mu0), np.asarray(p.tau0)) - logn(s, np.asarray(p.m0), np.asarray(p.s0)) for s in start]
    assert np.allclose(init, want, rtol=1e-12, atol=1e-12)
    assert np.all(path_weights_numpy(p, x, np.asarray(p.m0), 5, 2)[0] == 0.0)
    assert np.isclose(float(gauss_logpdf(np.array([0.3]), 1.0, 0.5)[0]), -0.5 * 0.49 / 0.5 - 0.5 * np.log(2.0 * np.pi * 0.5), rtol=1e-14)


def test_path_weights_record():
    rng = np.random.default_rng(4)
    n = 200
    w = PathWeights(rng.standard_normal(n), rng.standard_normal(n), 3.0 * rng.standard_normal(n))
    assert len(w) == n and np.array_equal(w.log_w, w.init + w.path + w.obs) and w.paths is None
    assert w.log_evidence() >= w.log_w.mean()
    assert np.isclose(w.log_evidence(), np.log(np.mean(np.exp(w.log_w))), rtol=1e-13)
    assert 1.0 <= w.ess() <= n
    low = PathWeights(np.zeros(n), -700.0 + rng.standard_normal(n), np.full(n, -50.0))
    assert np.isfinite(low.log_evidence()) and -760.0 < low.log_evidence() < -740.0 and low.log_evidence() >= low.log_w.mean()
    assert 1.0 <= low.ess() <= n
    flat = PathWeights(np.zeros(n), np.full(n, -3.0), np.full(n, -700.0))
    assert flat.ess() == n and np.isclose(flat.log_evidence(), -703.0, rtol=1e-15)
    assert np.array_equal(flat.resample(1), np.arange(n))
    # resampling: deterministic in its seed; one dominant weight takes every index
    a, b = w.resample(9), w.resample(9)
    assert a.shape == (n,) and np.array_equal(a, b) and a.min() >= 0 and a.max() < n and np.all(np.diff(a) >= 0)
    heavy = np.full(n, -1000.0)
    heavy[17] = 0.0
    one = PathWeights(np.zeros(n), heavy, np.zeros(n))
    assert np.all(one.resample(3) == 17) and np.isclose(one.ess(), 1.0, rtol=1e-15)
    # counts follow the weights: systematic resampling gives floor(n w) or ceil(n w) copies
    wn = np.exp(w.log_w - w.log_w.max())
    wn /= wn.sum()
    counts = np.bincount(a, minlength=n)
    assert np.all(np.abs(counts - n * wn) < 1.0 + 1e-9)
    # the self-normalised mean
    vals = rng.standard_normal((n, 3, 2))
    assert np.allclose(w.mean(vals), np.einsum("i,ijk->jk", wn, vals), rtol=1e-13, atol=1e-15)
    assert np.allclose(flat.mean(vals), vals.mean(axis=0), rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        PathWeights(np.zeros(3), np.zeros(4), np.zeros(3))


def test_symbol_and_prototype():
    assert "vgpa_sample_paths_weighted" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_sample_paths_weighted\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, "
                    "uint64_t seed, double* out_or_null, double* start_or_null, double* logw")


def test_python_surface():
    for owner, name, params in [(va.Context, "sample_paths_weighted", ["n_paths", "seed", "stride", "x", "x0", "paths"]),
                                (va.VarGP, "importance_weights", ["n_paths", "seed", "x", "x0", "stride"]),
                                (va.ProblemBatch, "importance_weights", ["n_paths", "seed", "x", "x0", "stride"])]:
        fn = getattr(owner, name, None)
        assert callable(fn), (owner.__name__, name)
        assert list(inspect.signature(fn).parameters)[1:] == params, (owner.__name__, name)
    sig = inspect.signature(va.Context.sample_paths_weighted).parameters
    assert sig["stride"].default == 1 and sig["paths"].default is True
    assert inspect.signature(va.VarGP.importance_weights).parameters["stride"].default is None
    assert va.PathWeights is PathWeights
    for name in ("log_evidence", "ess", "resample", "mean"):
        assert callable(getattr(PathWeights, name))
