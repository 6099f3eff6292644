"""
The smoothing moments on the grid under the particle filter's genealogy (vgpa_particle_moments): the numpy restatement, its checks against
the filter it rides on, against the backward recursion of vgpa_amd.particles.descendant_weights, against stored paths and against the exact
smoother of a linear chain, the record SmoothingMoments and the host-side surface.

The restatement is the reference of tests/test_particle_moments.py.  It is the walk of particle_ref.FilterWalk in which every slot carries its
whole path: x_i(k), the state of slot i as the walk arrives at k, is appended before the resampling decision at k, and a resampling copies
the paths through the same `anc` as the states (the forward algorithm).  With W = w / sum w of the final weights,
    M1[k] = sum_i W_i path_i(k),   M2[k] = sum_i W_i path_i(k)^2,   A1[k] = sum_i W_i |path_i(k)|   (the scale of M1's rounding).
The device computes the same numbers the other way round (the weights pushed backwards, descendant_weights); that the two agree is
test_backward_recursion_is_the_forward_algorithm.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import ParticleFilterResult, SmoothingMoments, descendant_weights
from conftest import ROOT
from particle_ref import FilterWalk
from test_particle_filter_cpu import SEED, case, particle_filter_numpy
from test_path_weights_cpu import FIXTURES, path_weights_numpy
from test_sample_paths_cpu import sample_paths_numpy


def lineage_paths(problem, x, x0, n, seed, ess_fraction, index=0):
    """(the finished walk, paths (n, Np, D)): every slot carries its whole path; a resampling copies the paths as it copies the states"""
    walk = FilterWalk(problem, x, x0, n, seed, ess_fraction, index)
    paths = np.zeros((n, walk.n_pts, walk.d))
    for event, i in walk:
        if event in ("start", "step"):
            paths[:, i] = walk.state
        elif event == "gather":
            paths = paths[walk.anc]
    return walk, paths


def final_weights(lw):
    """W = w / sum w of the final log-weights"""
    w = np.exp(lw - lw.max())
    return w / w.sum()


def lineage_moments(walk, paths):
    """m1 / m2 / a1 (Np, D) and lineage_ess (M + 1,) of a finished walk and the paths it carried"""
    w = final_weights(walk.lw)
    table = descendant_weights(walk.lw, walk.ancestors, walk.resampled) if walk.obs_t.size else w[None, :]
    return dict(m1=np.einsum("i,ikd->kd", w, paths), m2=np.einsum("i,ikd->kd", w, paths * paths),
                a1=np.einsum("i,ikd->kd", w, np.abs(paths)), lineage_ess=1.0 / np.sum(table * table, axis=1))


def particle_moments_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`, every slot carrying its path.  Returns FilterWalk.record's dict with m1 / m2 / a1
    (Np, D) and lineage_ess (M + 1,)."""
    walk, paths = lineage_paths(problem, x, x0, n, seed, ess_fraction, index)
    return walk.record(**lineage_moments(walk, paths))


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """the restatement of a case of test_particle_filter_cpu.case, computed once per process and shared by the CPU and GPU tests (read-only)"""
    q, x, x0 = case(tag)
    return particle_moments_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p", "quiet_l96d12"])
def test_same_walk_as_the_filter(tag):
    q, x, x0 = case(tag)
    for start in (None, x0):
        for frac in (0.0, 0.5, 1.0):
            got = particle_moments_numpy(q, x, start, 17, SEED, frac)
            want = particle_filter_numpy(q, x, start, 17, SEED, frac)
            for key in ("lw", "state", "ess", "resampled", "ancestors"):
                assert np.array_equal(got[key], want[key]), (tag, frac, key)
            assert np.array_equal(got["clouds"], want["clouds"]) and got["margins"] == want["margins"]


def test_descendant_weights_on_a_hand_made_table():
    """against the weighted bincount of lineages(): clouds that hold their own slot number make lineages() return, for every final slot,
    the slot it descends from at each observation"""
    anc = np.array([[0, 0, 2, 3], [0, 1, 2, 3], [0, 1, 3, 3]])
    flags = [1, 0, 1]
    lw = np.log(np.array([0.1, 0.2, 0.3, 0.4])) - 700.0
    clouds = np.tile(np.arange(4.0)[None, :, None], (3, 1, 1))
    rec = ParticleFilterResult(lw, np.zeros((4, 1)), [2.0, 4.0, 1.5], flags, anc, clouds)
    from_slot = rec.lineages()[..., 0].astype(int)      # (n, M)
    got = descendant_weights(lw, anc, flags)
    assert got.shape == (4, 4) and np.allclose(got[3], [0.1, 0.2, 0.3, 0.4], rtol=1e-13)
    for j in range(3):
        assert np.allclose(got[j], np.bincount(from_slot[:, j], weights=got[3], minlength=4), rtol=1e-14, atol=0.0), j
    assert np.array_equal(got[2], [got[3][0], got[3][1], 0.0, got[3][2] + got[3][3]]) and np.array_equal(got[1], got[2])
    assert np.array_equal(got[0], [got[1][0] + got[1][1], 0.0, got[1][2], got[1][3]])
    assert np.array_equal(rec.smoothing_weights(), got)
    assert np.allclose(got.sum(axis=1), 1.0, rtol=1e-14)
    with pytest.raises(ValueError):
        ParticleFilterResult(lw, np.zeros((4, 1)), [2.0], [0]).smoothing_weights()
    with pytest.raises(ValueError):
        descendant_weights(lw, anc, [1, 0])


@pytest.mark.parametrize("tag", ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p", "quiet_l96d17"])
def test_backward_recursion_is_the_forward_algorithm(tag):
    """descendant_weights on the restatement's histories, applied to its clouds, gives the moments the carried paths give at the
    observation indices; both are sums of at most n products of a weight and a state, each rounded to 1e-16: 1e-12 of sum W |x| holds
    for every n used here"""
    q, x, x0 = case(tag)
    worst = 0.0
    for start in (None, x0):
        for n, frac in ((17, 0.5), (65, 1.0), (65, 0.5)):
            ref = particle_moments_numpy(q, x, start, n, SEED, frac)
            table = descendant_weights(ref["lw"], ref["ancestors"], ref["resampled"])
            for j, t in enumerate(ref["obs_t"]):
                m1, m2 = table[j] @ ref["clouds"][j], table[j] @ ref["clouds"][j] ** 2
                worst = max(worst, float(np.max(np.abs(m1 - ref["m1"][t]) / ref["a1"][t])), float(np.max(np.abs(m2 - ref["m2"][t]) / ref["m2"][t])))
            rec = ParticleFilterResult(ref["lw"], ref["state"], ref["ess"], ref["resampled"], ref["ancestors"], ref["clouds"])
            assert np.allclose(rec.mean(rec.lineages()), ref["m1"][ref["obs_t"]], rtol=0.0, atol=1e-12 * float(ref["a1"].max()))
    print(tag, "worst backward against forward, relative to sum W |x| (M1) and M2:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("tag", FIXTURES)
def test_without_resampling_it_is_the_reweighted_stored_paths(tag):
    """ess_fraction = 0: the moments are the weighted mean of sample_paths_numpy's paths under path_weights_numpy's weights.  The two
    log-weights agree to 1e-12 (1 + scale) (test_particle_filter_cpu asserts it), so the normalised weights agree to twice that,
    relatively, and so do sums of non-negative terms of them"""
    q, x, x0 = case(tag)
    worst = 0.0
    for start in (None, x0):
        ref = particle_moments_numpy(q, x, start, 9, SEED, 0.0)
        init, path, obs, scale = path_weights_numpy(q, x, start, 9, SEED)
        paths = sample_paths_numpy(q, "posterior", x, start, 9, 1, SEED)
        lw = init + path + obs
        w = np.exp(lw - lw.max())
        w = w / w.sum()
        bound = 2e-12 * (1.0 + float(scale.max())) + 1e-14
        m1, m2, a1 = np.einsum("i,ikd->kd", w, paths), np.einsum("i,ikd->kd", w, paths * paths), np.einsum("i,ikd->kd", w, np.abs(paths))
        worst = max(worst, float(np.max(np.abs(ref["m1"] - m1) / a1)) / bound, float(np.max(np.abs(ref["m2"] - m2) / m2)) / bound)
        assert np.allclose(ref["lineage_ess"], 1.0 / np.sum(w * w), rtol=10 * bound)
    print(tag, "worst deviation from the reweighted stored paths, in units of its bound:", worst)
    assert worst <= 1.0


# ---- the exact anchor: a linear-Gaussian chain ---------------------------------------------------------------------------------------------
def rts_marginals(q):
    """exact E[x_k | y] and Var[x_k | y] of the chain x_k = a x_{k-1} + N(0, sigma dt), a = 1 - theta dt, x_0 ~ N(mu0, tau0),
    y_j = x_{t_j} + N(0, r): the Kalman filter and the Rauch-Tung-Striebel recursion, as test_particle_statistics_cpu.rts_expectations"""
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
    for k in range(n - 1, 0, -1):
        j = pf[k - 1] * a / pp[k]
        ms[k - 1] = mf[k - 1] + j * (ms[k] - mp[k])
        ps[k - 1] = pf[k - 1] + j * j * (ps[k] - pp[k])
    return ms, ps


def test_rts_anchor():
    """4096 particles, 16 seeds: the seed-mean of the smoothing mean and variance within 4 standard errors of the exact ones at grid index 0,
    an observation index, a mid-gap index and Np - 1"""
    q, _, _ = case("ou_euler")
    n = int(q.n_pts)
    x = np.concatenate((np.full(n, float(q.theta)), np.zeros(n)))      # A_t = theta, b_t = 0: the proposal is the model
    ms, ps = rts_marginals(q)
    t = np.asarray(q.obs_t, dtype=int).ravel()
    at = np.array([0, t[0], (t[0] + t[1]) // 2, n - 1])      # index 0, an observation, the middle of the gap behind it, the last index
    assert at[2] not in t and 0 < at[1] < at[2] < n - 1
    runs = [particle_moments_numpy(q, x, None, 4096, s, 0.5) for s in range(1, 17)]
    mean = np.array([r["m1"][at, 0] for r in runs])
    var = np.array([r["m2"][at, 0] - r["m1"][at, 0] ** 2 for r in runs])
    se_m, se_v = mean.std(axis=0, ddof=1) / 4.0, var.std(axis=0, ddof=1) / 4.0
    print("grid indices", at, " lineage ESS of the stretches (first seed):", np.round(runs[0]["lineage_ess"], 1))
    print("exact mean", ms[at], " seed-mean", mean.mean(axis=0), " standard error", se_m)
    print("exact var ", ps[at], " seed-mean", var.mean(axis=0), " standard error", se_v)
    assert np.all(np.abs(mean.mean(axis=0) - ms[at]) <= 4.0 * se_m)
    assert np.all(np.abs(var.mean(axis=0) - ps[at]) <= 4.0 * se_v)


# ---- the seeds of the GPU tests ------------------------------------------------------------------------------------------------------------
def test_margin_condition_of_the_runs_not_cleared_elsewhere():
    """tests/test_particle_moments.py reuses the (case, n, seed) that test_particle_filter_cpu.test_margin_condition clears; the two it
    shares with the sibling GPU tests beyond those -- the cached-x cases (9 particles, seed 4, the last problem) and the ProblemBatch
    members (17 particles, SEED_BATCH) -- keep every threshold at least 1e-7 S away from every prefix sum as well"""
    from helpers import build_problem
    from test_particle_filter import CACHE_CASES
    from test_particle_filter_cpu import MARGIN, SEED_BATCH
    from test_path_weights import _fields
    from test_problem_batch import _datasets
    smallest = np.inf
    for name, method, d, tf, nb in CACHE_CASES:
        _, probs, xs = _datasets(name, method, tf, d, nb, False)
        margins = particle_filter_numpy(probs[nb - 1], xs[nb - 1], None, 9, 4, 0.5, index=nb - 1)["margins"]
        smallest = min([smallest] + margins)
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    for k, p in enumerate(ps):
        margins = particle_filter_numpy(_fields(p["vgp"]), p["vgp"].initialization(), None, 17, SEED_BATCH, 0.5, index=k)["margins"]
        smallest = min([smallest] + margins)
    print("smallest margin:", smallest)
    assert smallest >= MARGIN


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    mom = np.arange(4 * 2 * 3, dtype=float).reshape(4, 2, 3) + 1.0
    mom[:, 1] += mom[:, 0] ** 2
    rec = SmoothingMoments([-700.0, -701.0], mom, 3, 11, [0, 4, 10], [1.5, 1.6, 1.7, 1.8], [2.0, 1.0, 1.5], [1, 0, 0])
    assert len(rec) == 2 and np.array_equal(rec.grid, [0, 3, 6, 9]) and rec.resampled.dtype == bool
    assert np.array_equal(rec.mean, mom[:, 0]) and np.array_equal(rec.second, mom[:, 1])
    assert np.array_equal(rec.var, mom[:, 1] - mom[:, 0] ** 2) and np.allclose(rec.std ** 2, rec.var, rtol=1e-14)
    # index 0 lies in stretch 0 (k <= t_0 = 0), 3 in stretch 1 (0 < k <= 4), 6 and 9 in stretch 2 (4 < k <= 10)
    assert np.array_equal(rec.lineage_ess_on_grid(), [1.5, 1.6, 1.7, 1.7])
    assert np.isclose(rec.log_evidence(), -700.0 + np.log((1.0 + np.exp(-1.0)) / 2.0))
    one = SmoothingMoments([0.0], mom[:, :, :1], 3, 11, [], [1.0], single_dim=True)
    assert one.mean.shape == one.var.shape == one.std.shape == (4,) and np.array_equal(one.lineage_ess_on_grid(), np.ones(4))
    neg = SmoothingMoments([0.0], np.array([[[1.0], [1.0 - 1e-16]]]), 5, 3, [], [1.0])
    assert neg.var[0, 0] < 0.0 and neg.std[0, 0] == 0.0      # (the variance as it comes; the deviation clipped)
    for bad in (lambda: SmoothingMoments([], mom, 3, 11, [], [1.0]), lambda: SmoothingMoments([0.0], mom, 2, 11, [], [1.0]),
                lambda: SmoothingMoments([0.0], mom, 0, 11, [], [1.0]), lambda: SmoothingMoments([0.0], mom, 3, 11, [1, 2], [1.0]),
                lambda: SmoothingMoments([0.0], mom, 3, 11, [], [1.0], [1.0], [])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_moments" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_moments\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed, "
                    "double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, "
                    "double* moments, double* lineage_ess_or_null, double* ess_or_null, int32_t* resampled_or_null")


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0", "prior"]),
                          (va.VarGP, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"]),
                          (va.ProblemBatch, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"])]:
        fn = getattr(owner, "particle_moments", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["stride"].default == 1
    assert va.SmoothingMoments is SmoothingMoments and "SmoothingMoments" in va.__all__
    for name in ("mean", "second", "var", "std", "grid"):
        assert isinstance(getattr(SmoothingMoments, name), property), name
    for name in ("lineage_ess_on_grid", "log_evidence"):
        assert callable(getattr(SmoothingMoments, name))
    assert callable(descendant_weights) and callable(ParticleFilterResult.smoothing_weights)
