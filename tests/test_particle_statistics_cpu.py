"""
The path statistics of the particle filter's lineages (vgpa_particle_statistics): the numpy restatement, its checks against the filter it
rides on, against stored paths and against the exact smoother of a linear chain, the record PathStatistics and the host-side surface.

The restatement is the reference of tests/test_particle_statistics.py.  It is the walk of particle_ref.FilterWalk with a row (Q, G, H) per
slot,
    Q_j += r_j^2 / dt,  G_j += phi_j r_j,  H_j += dt phi_j^2,  r = dt (g - f_theta(x_{k-1})) + eta_k,  phi_j = df_j / dtheta_a(j) at x_{k-1},
and, per entry, the scale sum_k |increment_k|.  A resampling copies rows and scales through the same `anc` as the states.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import PathStatistics
from conftest import ROOT
from particle_ref import FilterWalk
from test_particle_filter_cpu import SEED, case, particle_filter_numpy
from test_path_weights_cpu import _sigma_diag
from test_sample_paths_cpu import model_drift, sample_paths_numpy

THETA_CASES = ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p"]


def model_phi(model, x):
    """phi_j = df_j / dtheta_a(j) at x (n, D)"""
    if model == "OU":
        return -x
    if model == "DW":
        return 4.0 * x
    if model == "L63":
        return np.stack((x[:, 1] - x[:, 0], x[:, 0], -x[:, 2]), axis=1)
    return np.ones_like(x)


def particle_statistics_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`, the rows carried along.  Returns FilterWalk.record's dict with rows (n, 3, D) and
    scale (n, 3, D)."""
    walk = FilterWalk(problem, x, x0, n, seed, ess_fraction, index)
    dt = walk.dt
    rows, scale = np.zeros((n, 3, walk.d)), np.zeros((n, 3, walk.d))
    for event, _ in walk:
        if event == "step":
            res, phi = dt * walk.dd + walk.eta, model_phi(problem.model, walk.prev)
            step = np.stack((res * res / dt, phi * res, dt * (phi * phi)), axis=1)
            rows, scale = rows + step, scale + np.abs(step)
        elif event == "gather":
            rows, scale = rows[walk.anc], scale[walk.anc]
    return walk.record(rows=rows, scale=scale)


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """the restatement of a case of test_particle_filter_cpu.case, computed once per process and shared by the CPU and GPU tests (read-only)"""
    q, x, x0 = case(tag)
    return particle_statistics_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


def weighted_mean(lw, rows):
    w = np.exp(lw - np.max(lw))
    return np.tensordot(w, rows, axes=(0, 0)) / np.sum(w)


def record(problem, ref):
    return PathStatistics(ref["lw"], weighted_mean(ref["lw"], ref["rows"]), float(problem.dt), int(problem.n_pts) - 1, problem.model,
                          ref["ess"], ref["resampled"], ref["rows"])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", THETA_CASES + ["l96d17_rk4_p"])
def test_same_walk_as_the_filter(tag):
    q, x, x0 = case(tag)
    for start in (None, x0):
        for frac in (0.0, 0.5, 1.0):
            got = particle_statistics_numpy(q, x, start, 17, SEED, frac)
            want = particle_filter_numpy(q, x, start, 17, SEED, frac)
            for key in ("lw", "state", "ess", "resampled"):
                assert np.array_equal(got[key], want[key]), (tag, frac, key)
            assert got["margins"] == want["margins"]


@pytest.mark.parametrize("tag", THETA_CASES)
def test_rows_against_stored_paths(tag):
    """ess_fraction = 0: the rows are the statistics of the stored paths, r = (x_k - x_{k-1}) - dt f(x_{k-1})"""
    q, x, x0 = case(tag)
    dt, theta = float(q.dt), np.asarray(q.theta, dtype=float)
    worst = 0.0
    for start in (None, x0):
        got = particle_statistics_numpy(q, x, start, 9, SEED, 0.0)
        paths = sample_paths_numpy(q, "posterior", x, start, 9, 1, SEED)
        want = np.zeros_like(got["rows"])
        for k in range(1, int(q.n_pts)):
            prev = paths[:, k - 1]
            res, phi = (paths[:, k] - prev) - dt * model_drift(q.model, theta, prev), model_phi(q.model, prev)
            want += np.stack((res * res / dt, phi * res, dt * (phi * phi)), axis=1)
        worst = max(worst, float(np.max(np.abs(got["rows"] - want) / (got["scale"] + 1e-300))))
    print(tag, "worst |rows - stored-path statistics| / scale =", worst)
    assert worst <= 1e-12


# ---- the theta step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", THETA_CASES)
def test_theta_step_maximises_the_q_function(tag):
    q, x, _ = case(tag)
    rec = record(q, particle_statistics_numpy(q, x, None, 65, SEED, 0.5))
    sg = _sigma_diag(q).diagonal()
    theta = np.atleast_1d(np.asarray(q.theta, dtype=float))
    step, score = rec.theta_step(sg), rec.score(sg)
    assert step.shape == score.shape == rec.information(sg).shape == (rec.n_theta,) == theta.shape
    best = rec.expected_loglik(theta + step, sg, theta)
    for a in range(rec.n_theta):
        for eps in (1e-3, -1e-3, 0.5, -0.5):
            e = np.zeros(rec.n_theta)
            e[a] = eps
            assert rec.expected_loglik(theta + step + e, sg, theta) < best, (tag, a, eps)
        # the Q-function is quadratic in theta': the central difference over +-1 is its gradient up to rounding
        e = np.zeros(rec.n_theta)
        e[a] = 1.0
        grad = 0.5 * (rec.expected_loglik(theta + step + e, sg, theta) - rec.expected_loglik(theta + step - e, sg, theta))
        exact = score[a] - step[a] * rec.information(sg)[a]
        print(tag, a, "score", score[a], "step", step[a], "dQ/dtheta at the maximiser: difference", grad, "closed form", exact)
        assert abs(exact) <= 1e-9 * abs(score[a])
        assert abs(grad) <= 1e-9 * abs(score[a]) + 1e-12 * abs(best)      # (the rounding of the two Q values themselves)
    assert best > rec.expected_loglik(theta, sg, theta)
    if tag == "l63_euler_p":
        assert np.allclose(rec.theta_step(3.0 * sg), step, rtol=1e-14)


def test_pooled_step_maximises_the_summed_q_function():
    q, x, _ = case("dw_euler_p")
    sg = _sigma_diag(q).diagonal()
    theta = np.atleast_1d(np.asarray(q.theta, dtype=float))
    recs = [record(q, particle_statistics_numpy(q, x, None, 65, s, 0.5)) for s in (1, 2, 3)]
    step = sum(r.score(sg) for r in recs) / sum(r.information(sg) for r in recs)
    total = lambda t: sum(r.expected_loglik(t, sg, theta) for r in recs)      # noqa: E731
    best = total(theta + step)
    for eps in (1e-3, -1e-3, 0.5, -0.5):
        assert total(theta + step + eps) < best
    assert any(abs(r.theta_step(sg)[0] - step[0]) > 1e-6 for r in recs)


# ---- the exact anchor: a linear-Gaussian chain ---------------------------------------------------------------------------------------------
def rts_expectations(q):
    """exact E[sum_k phi r | y] and E[sum_k dt phi^2 | y] of the chain x_k = a x_{k-1} + N(0, sigma dt), a = 1 - theta dt, x_0 ~ N(mu0, tau0),
    y_j = x_{t_j} + N(0, r): phi = -x_{k-1}, r = x_k - a x_{k-1}"""
    dt, n = float(q.dt), int(q.n_pts)
    a, qv, r = 1.0 - float(q.theta) * dt, float(q.sigma) * dt, float(np.ravel(q.obs_noise)[0])
    at = {int(t): float(y) for t, y in zip(np.ravel(q.obs_t), np.ravel(q.obs_y))}
    mp, pp, mf, pf = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(n):
        mp[k], pp[k] = (float(np.ravel(q.mu0)[0]), float(np.ravel(q.tau0)[0])) if k == 0 else (a * mf[k - 1], a * a * pf[k - 1] + qv)
        mf[k], pf[k] = mp[k], pp[k]
        if k in at:
            gain = pp[k] / (pp[k] + r)
            mf[k], pf[k] = mp[k] + gain * (at[k] - mp[k]), (1.0 - gain) * pp[k]
    ms, ps = mf.copy(), pf.copy()
    e_g = e_h = 0.0
    for k in range(n - 1, 0, -1):
        j = pf[k - 1] * a / pp[k]
        ms[k - 1] = mf[k - 1] + j * (ms[k] - mp[k])
        ps[k - 1] = pf[k - 1] + j * j * (ps[k] - pp[k])
        cross = j * ps[k] + ms[k - 1] * ms[k]
        second = ps[k - 1] + ms[k - 1] ** 2
        e_g += -(cross - a * second)
        e_h += dt * second
    return e_g, e_h


def test_rts_anchor():
    q, _, _ = case("ou_euler")
    n = int(q.n_pts)
    x = np.concatenate((np.full(n, float(q.theta)), np.zeros(n)))      # A_t = theta, b_t = 0: the proposal is the model
    e_g, e_h = rts_expectations(q)
    runs = [particle_statistics_numpy(q, x, None, 4096, s, 0.5) for s in range(1, 17)]
    means = np.array([weighted_mean(r["lw"], r["rows"])[1:, 0] for r in runs])
    se = means.std(axis=0, ddof=1) / 4.0
    print("exact E[G], E[H]:", e_g, e_h, " seed-mean:", means.mean(axis=0), " standard error:", se)
    assert abs(means[:, 0].mean() - e_g) <= 4.0 * se[0]
    assert abs(means[:, 1].mean() - e_h) <= 4.0 * se[1]


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    mean = np.array([[8.0, 2.0, 4.0], [1.0, -2.0, 3.0], [2.0, 4.0, 1.5]])
    sg = np.array([2.0, 4.0, 0.5])
    one = PathStatistics(np.zeros(4), mean, 0.1, 10, "L96", [3.0], [1])
    assert len(one) == 4 and one.n_theta == 1 and one.rows is None and one.resampled.dtype == bool and one.dim_d == 3
    assert all(np.array_equal(a, b) for a, b in zip(one.expected(), mean))
    assert np.allclose(one.score(sg), [0.5 - 0.5 + 6.0]) and np.allclose(one.information(sg), [1.0 + 1.0 + 3.0])
    assert np.allclose(one.theta_step(sg), [6.0 / 5.0])
    want = -0.5 * (np.sum((mean[0] - 2.0 * 0.5 * mean[1] + 0.25 * mean[2]) / sg) + 10 * np.sum(np.log(2.0 * np.pi * sg * 0.1)))
    assert np.isclose(one.expected_loglik(1.5, sg, 1.0), want, rtol=1e-15)
    three = PathStatistics(np.zeros(4), mean, 0.1, 10, "L63")
    assert three.n_theta == 3 and np.allclose(three.score(sg), mean[1] / sg) and np.allclose(three.theta_step(sg), mean[1] / mean[2])
    delta = np.array([0.5, -1.0, 2.0])
    want = -0.5 * (np.sum((mean[0] - 2.0 * delta * mean[1] + delta ** 2 * mean[2]) / sg) + 10 * np.sum(np.log(2.0 * np.pi * sg * 0.1)))
    assert np.isclose(three.expected_loglik(np.ones(3) + delta, sg, np.ones(3)), want, rtol=1e-15)
    assert np.isclose(PathStatistics([-700.0, -701.0], mean[:, :1], 0.1, 10, "OU").log_evidence(), -700.0 + np.log((1.0 + np.exp(-1.0)) / 2.0))
    for bad in (lambda: PathStatistics([], mean, 0.1, 10, "L96"), lambda: PathStatistics(np.zeros(4), mean[:2], 0.1, 10, "L96"),
                lambda: PathStatistics(np.zeros(4), mean, 0.1, 10, "NONE"), lambda: PathStatistics(np.zeros(4), mean[:, :2], 0.1, 10, "L63"),
                lambda: PathStatistics(np.zeros(4), mean, 0.1, 10, "L96", rows=np.zeros((3, 3, 3))),
                lambda: PathStatistics(np.zeros(4), mean, 0.1, 10, "L96", [1.0], [])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_statistics" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_statistics\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed, double ess_fraction, "
                    "const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* stats_or_null, "
                    "double* mean_or_null, double* ess_or_null, int32_t* resampled_or_null")


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "ess_fraction", "x", "x0", "prior", "per_particle"]),
                          (va.VarGP, ["n_paths", "seed", "ess_fraction", "x", "x0", "per_particle"]),
                          (va.ProblemBatch, ["n_paths", "seed", "ess_fraction", "x", "x0", "per_particle"])]:
        fn = getattr(owner, "particle_statistics", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["per_particle"].default is False
    for owner in (va.VarGP, va.ProblemBatch):
        sig = inspect.signature(owner.particle_fit_theta).parameters
        assert list(sig)[1:7] == ["n_paths", "seed", "iters", "ess_fraction", "refit", "pooled"], owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["refit"].default is True and sig["pooled"].default is False
        assert "Sigma" in owner.particle_fit_theta.__doc__ or "Sigma" in va.ProblemBatch.particle_fit_theta.__doc__
    assert va.PathStatistics is PathStatistics and "PathStatistics" in va.__all__
    for name in ("expected", "score", "information", "theta_step", "expected_loglik", "log_evidence"):
        assert callable(getattr(PathStatistics, name))
    assert not any("sigma_step" in name or "sigma_mstep" in name for name in dir(PathStatistics))
