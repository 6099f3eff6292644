"""
The guided particle filter (vgpa_particle_filter): the numpy restatement, its checks against the importance weights it generalises and against
the exact evidence of a linear chain, the record ParticleFilterResult, the host-side surface, and the margin condition of the GPU tests.

The restatement is the reference of tests/test_particle_filter.py.  It is the walk of particle_ref.FilterWalk (the recursion, the resampling
rule and the margin are described there) and carries, per slot,

scale: sum_k |increment_k| of the path term as in path_weights_numpy; a resampling sets every slot's scale to the largest (the common
log-weight is made of all of them).
"""
import dataclasses
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import ParticleFilterResult
from conftest import ROOT, load_golden
from oracle import vgpa_oracle as vo
from particle_ref import FilterWalk
from test_gpu_edge_cases import make_problem
from test_path_weights_cpu import FIXTURES, TAGS, path_weights_numpy

SEED = 7                         # (seed 5 leaves l96d5 and two quiet cases a margin of 2.5e-8 .. 6.6e-8 at n = 300: another seed, the same bound)
SEED_BATCH = 9                   # ... and the batch cases' (seed 7: 3.1e-8)
SIZES = (17, 65, 300)            # (and 1, which has nothing to decide: its one ancestor is 0)
FRACTIONS = (0.5, 1.0)
QUIET = ["quiet_l96d12", "quiet_l96d17", "quiet_l96d40"]
MARGIN = 1e-7
OU_BIG = ("ou_euler", "drawn", 4096, 0.5, 436)      # the one large run of the GPU tests: 4096 thresholds among 4096 prefix sums keep the margin at
                                                    # about one seed in a thousand; 436 is the first that does (two resamplings)
PLACEMENTS = [(0, 7, 20), (10, 11, 12), (0, 1, 39, 40)]
BATCH_TIMES = [np.array([0, 6, 13, 27, 40]), np.array([3, 4, 30, 39]), np.array([9, 21, 22])]


def particle_filter_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`.  Returns FilterWalk.record's dict with scale (n,) and init (n,)."""
    walk = FilterWalk(problem, x, x0, n, seed, ess_fraction, index)
    scale = np.zeros(n)
    for event, _ in walk:
        if event == "step":
            scale = scale + np.abs(walk.inc)
        elif event == "gather":
            scale = np.full(n, scale.max())
    return walk.record(scale=scale, init=walk.init)


def log_mean_exp(lw):
    top = np.max(lw)
    return float(top + np.log(np.sum(np.exp(lw - top))) - np.log(lw.size))


# ---- the cases of the GPU tests: oracle problems (or anything with their fields), built once ---------------------------------------------
def _given(q):
    return np.reshape(np.asarray(q.m0, dtype=float), q.dim_d) + 0.1


@functools.lru_cache(maxsize=None)
def case(tag):
    """(problem, x, given start) of a tag: a fixture, "l96d4" / "l96d5" / "l96d64" of test_path_weights.py, or a quiet case -- a Lorenz-96 fixture's
    grid with theta = 0, observations 0, A_t = I, b_t = 0 and every particle started at 0: the weights stay comparable, so that the clouds
    are partly resampled and partly carried on"""
    if tag in FIXTURES:
        z = load_golden(tag)
        q = vo.Problem.from_fixture(z)
        return q, np.asarray(z["x"], dtype=float), _given(q)
    if tag in QUIET:
        q = vo.Problem.from_fixture(load_golden({"quiet_l96d12": "l96d12_euler_p", "quiet_l96d17": "l96d17_rk4_p", "quiet_l96d40": "l96d40_rk4_p"}[tag]))
        d, n = int(q.dim_d), int(q.n_pts)
        q = dataclasses.replace(q, theta=0.0, obs_y=np.zeros((np.asarray(q.obs_t).size, d)))
        return q, np.concatenate((np.tile(np.eye(d).ravel(), n), np.zeros(n * d))), np.zeros(d)
    if tag == "l96d64":
        from helpers import build_problem
        from test_path_weights import _fields
        v = build_problem("L96", "euler", 0.5, dim_d=64)["vgp"]
        x = v.initialization() + 0.05 * np.random.default_rng(3).standard_normal(v.dim_n * 64 * 65)
        q = _fields(v)
        return q, x, _given(q)
    assert tag in ("l96d4", "l96d5"), tag
    q, x = make_problem("L96", int(tag[4:]), 41, method="euler")
    return q, x, _given(q)


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """the restatement of a case, computed once per process and shared by the CPU and GPU tests (read-only)"""
    q, x, x0 = case(tag)
    return particle_filter_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


@functools.lru_cache(maxsize=None)
def placement_case(model, d, obs_at):
    q, x = make_problem(model, d, 41, method="euler", obs_at=list(obs_at))
    if model == "L63":          # (as in test_path_weights.py: keep the Lorenz-63 chain near its data)
        x = np.concatenate((x[:41 * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(41, axis=0).ravel()))
    return q, x


@functools.lru_cache(maxsize=None)
def batch_case(model, d, first):
    """three problems with their own observation times and counts, theta, isotropic Sigma, prior moments, dense R and H; `first`: the seed
    of the first problem (another one swaps the neighbours of the last problem for different ones)"""
    rng = np.random.default_rng(11)
    probs, xs = [], []
    for k in range(3):
        q, x = make_problem(model, d, 41, method="euler", seed=(first + k) if k < 2 else 22, obs_at=list(BATCH_TIMES[k]))
        if model == "L63":
            x = np.concatenate((x[:41 * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(41, axis=0).ravel()))
        theta = np.asarray(q.theta, dtype=float) * (1.0 + 0.05 * k)
        from test_gpu_edge_cases import spd
        q = dataclasses.replace(q, theta=theta if theta.ndim else float(theta), sigma=(3.0 + 0.4 * k) * np.eye(d),
                                s0=np.asarray(q.s0) * (1.0 + 0.1 * k), obs_noise=spd(rng, d, 1.0 + 0.2 * k, 0.2),
                                obs_h=np.eye(d) + 0.1 * rng.standard_normal((d, d)))
        probs.append(q)
        xs.append(x)
    return probs, np.stack(xs)


def gpu_runs():
    """every restatement the GPU tests compare ancestors with, as (label, thunk)"""
    runs = []
    for tag in TAGS + QUIET:
        for start in (("given",) if tag in QUIET else ("given", "drawn")):
            for n in SIZES:
                for frac in FRACTIONS:
                    runs.append(((tag, start, n, frac), functools.partial(reference, tag, start, n, frac)))
    runs.append((OU_BIG, functools.partial(reference, *OU_BIG)))
    for model, d in (("L63", 3), ("L96", 12)):
        for obs_at in PLACEMENTS:
            q, x = placement_case(model, d, obs_at)
            for x0 in (None, _given(q)):
                runs.append((("placement", model, obs_at, x0 is None), functools.partial(particle_filter_numpy, q, x, x0, 17, SEED, 1.0)))
        for first in (20, 50):
            probs, xs = batch_case(model, d, first)
            for k in range(3):
                runs.append((("batch", model, first, k), functools.partial(particle_filter_numpy, probs[k], xs[k], None, 40, SEED_BATCH, 0.5, index=k)))
    return runs


def test_margin_condition():
    """a condition on the cases, not a measurement of the device: every threshold of every resampling the GPU tests compare keeps a distance
    of at least 1e-7 S from every prefix sum (were a seed to fail, another seed is picked -- the bound stays)"""
    worst = {}
    for label, thunk in gpu_runs():
        margins = thunk()["margins"]
        if margins:
            group = label[0] if label[0] in ("placement", "batch") else ("quiet" if label[0] in QUIET else "fixtures")
            worst[group] = min(worst.get(group, np.inf), min(margins))
            assert min(margins) >= MARGIN, (label, min(margins))
    print("smallest margin per group:", worst)
    assert set(worst) == {"fixtures", "quiet", "placement", "batch"}


def test_quiet_cases_mix_the_decisions():
    kinds = set()
    for tag in QUIET:
        for n in (65, 300):
            ref = reference(tag, "given", n, 0.5)
            print(tag, n, "ESS / n at the observations:", np.round(ref["ess"] / n, 3), "resampled:", ref["resampled"])
            kinds |= set(ref["resampled"][:-1].tolist())
    assert kinds == {0, 1}


@pytest.mark.parametrize("tag", FIXTURES)
def test_without_resampling_it_is_the_importance_weights(tag):
    q, x, x0 = case(tag)
    worst = 0.0
    for start in (None, x0):
        got = particle_filter_numpy(q, x, start, 9, SEED, 0.0)
        init, path, obs, scale = path_weights_numpy(q, x, start, 9, SEED)
        worst = max(worst, float(np.max(np.abs(got["lw"] - (init + path + obs)) / (1.0 + scale))))
        assert not got["resampled"].any() and not got["margins"] and np.array_equal(got["scale"], scale)
        assert np.array_equal(got["ancestors"], np.tile(np.arange(9), (got["ess"].size, 1)))
        assert np.all(np.abs(got["init"] - init) <= 1e-12)
    print(tag, "worst |lw - (init + path + obs)| / (1 + scale) =", worst)
    assert worst <= 1e-12


def kalman_log_evidence(q):
    """exact log p(y) of the scalar chain x_k = (1 - theta dt) x_{k-1} + sqrt(sigma dt) xi, x_0 ~ N(mu0, tau0), y_j = x_{t_j} + N(0, r)"""
    a, qv, r = 1.0 - float(q.theta) * float(q.dt), float(q.sigma) * float(q.dt), float(np.ravel(q.obs_noise)[0])
    at = {int(t): float(y) for t, y in zip(np.ravel(q.obs_t), np.ravel(q.obs_y))}
    mean, var, total = float(np.ravel(q.mu0)[0]), float(np.ravel(q.tau0)[0]), 0.0
    for k in range(int(q.n_pts)):
        if k > 0:
            mean, var = a * mean, a * a * var + qv
        if k in at:
            s = var + r
            total += -0.5 * np.log(2.0 * np.pi * s) - 0.5 * (at[k] - mean) ** 2 / s
            gain = var / s
            mean, var = mean + gain * (at[k] - mean), (1.0 - gain) * var
    return total


def test_kalman_anchor():
    q, x, _ = case("ou_euler")
    exact = kalman_log_evidence(q)
    with_rs = np.array([log_mean_exp(particle_filter_numpy(q, x, None, 4096, s, 0.5)["lw"]) for s in range(1, 21)])
    without = np.array([log_mean_exp(particle_filter_numpy(q, x, None, 4096, s, 0.0)["lw"]) for s in range(1, 21)])
    print("exact", exact, " resampling at ESS < n/2: mean", with_rs.mean(), "sd", with_rs.std(ddof=1), " without: mean", without.mean(),
          "sd", without.std(ddof=1))
    assert abs(exact - (-2.671431)) <= 5e-6
    assert abs(with_rs.mean() - exact) <= 5.0 * with_rs.std(ddof=1) / np.sqrt(20.0)
    assert without.std(ddof=1) > with_rs.std(ddof=1)


def test_lineages_on_a_hand_made_table():
    clouds = np.arange(3 * 4 * 2, dtype=float).reshape(3, 4, 2)
    anc = np.array([[0, 0, 2, 3], [0, 1, 2, 3], [3, 3, 1, 0]])
    rec = ParticleFilterResult(np.zeros(4), np.zeros((4, 2)), [2.0, 4.0, 1.5], [1, 0, 1], anc, clouds)
    lin = rec.lineages()
    assert lin.shape == (4, 3, 2)
    # final slot 0: observation 2 from slot 3, carried on at observation 1, observation 0 from slot 3
    assert np.array_equal(lin[0], np.stack((clouds[0, 3], clouds[1, 3], clouds[2, 3])))
    # final slot 2: slot 1 at observations 2 and 1, which came from slot 0 at observation 0
    assert np.array_equal(lin[2], np.stack((clouds[0, 0], clouds[1, 1], clouds[2, 1])))
    assert np.array_equal(lin[3], np.stack((clouds[0, 0], clouds[1, 0], clouds[2, 0])))
    one = ParticleFilterResult(np.zeros(4), np.zeros(4), [2.0, 4.0, 1.5], [1, 0, 1], anc, clouds[..., 0])      # a 1-D model
    assert one.lineages().shape == (4, 3) and np.array_equal(one.lineages(), lin[..., 0])
    with pytest.raises(ValueError):
        ParticleFilterResult(np.zeros(4), np.zeros((4, 2)), [2.0], [0]).lineages()
    with pytest.raises(ValueError):
        ParticleFilterResult(np.zeros(4), np.zeros((3, 2)), [2.0], [0])


def test_record():
    rng = np.random.default_rng(4)
    lw = 3.0 * rng.standard_normal(50) - 700.0
    rec = ParticleFilterResult(lw, rng.standard_normal((50, 3)), [10.0, 20.0], [1, 0])
    assert len(rec) == 50 and rec.ancestors is None and rec.clouds is None and rec.resampled.dtype == bool
    assert np.isclose(rec.log_evidence(), log_mean_exp(lw), rtol=1e-15) and 1.0 <= rec.final_ess() <= 50.0
    assert np.isclose(rec.log_evidence(), va.PathWeights(np.zeros(50), lw, np.zeros(50)).log_evidence(), rtol=1e-15)
    w = np.exp(lw - lw.max())
    assert np.allclose(rec.mean(rec.state), (w / w.sum()) @ rec.state, rtol=1e-13)
    assert ParticleFilterResult(np.full(7, -3.0), np.zeros((7, 1)), [], []).final_ess() == 7.0


def test_symbol_and_prototype():
    assert "vgpa_particle_filter" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_filter\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed, double ess_fraction, "
                    "const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* ess_or_null, "
                    "int32_t* resampled_or_null, int32_t* ancestors_or_null, double* clouds_or_null")


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "ess_fraction", "x", "x0", "prior", "history"]),
                          (va.VarGP, ["n_paths", "seed", "ess_fraction", "x", "x0", "history"]),
                          (va.ProblemBatch, ["n_paths", "seed", "ess_fraction", "x", "x0", "history"])]:
        fn = getattr(owner, "particle_filter", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["history"].default is False
    assert va.ParticleFilterResult is ParticleFilterResult and "ParticleFilterResult" in va.__all__
    for name in ("log_evidence", "final_ess", "mean", "lineages"):
        assert callable(getattr(ParticleFilterResult, name))
