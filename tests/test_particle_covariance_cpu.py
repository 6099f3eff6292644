"""
The smoothing mean and full second-moment matrices on the grid under the particle filter's genealogy (vgpa_particle_covariance): the numpy
restatement, its checks against the restatement of the moments it extends, against the backward recursion of
vgpa_amd.particles.descendant_weights and against stored paths, the record SmoothingCovariance and the host-side surface.

The restatement is the reference of tests/test_particle_covariance.py.  It is test_particle_moments_cpu.particle_moments_numpy (the same
walk, test_particle_moments_cpu.lineage_paths: every slot carries its whole path through the resamplings), which returns in addition, with W = w / sum w of the final weights,
    second[k][a][b] = sum_i W_i path_i(k)[a] path_i(k)[b],   a2[k][a][b] = sum_i W_i |path_i(k)[a]| |path_i(k)[b]|   (the scale of its rounding).
The lower triangle is summed, (W x_a) x_b in slot order, and mirrored.
"""
import inspect
import os
import re
import functools

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import SmoothingCovariance, descendant_weights
from conftest import ROOT
from test_particle_filter_cpu import SEED, case
from test_particle_moments_cpu import final_weights, lineage_moments, lineage_paths, particle_moments_numpy
from test_path_weights_cpu import FIXTURES, path_weights_numpy
from test_sample_paths_cpu import sample_paths_numpy

WALK_TAGS = ["ou_euler", "l63_euler_p", "l96d12_euler_p", "l96d17_rk4_p", "quiet_l96d12"]      # (those of test_particle_moments_cpu)


def weighted_second(w, pts):
    """sum_i w_i pts[i][..., a] pts[i][..., b] for b <= a, (w x_a) x_b added in the order of i, mirrored: (n,), (n, K, D) -> (K, D, D)"""
    low = np.tril(np.einsum("ika,ikb->kab", w[:, None, None] * pts, pts))
    return low + np.transpose(np.tril(low, -1), (0, 2, 1))


def particle_covariance_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`, every slot carrying its path.  Returns particle_moments_numpy's dict and second / a2
    (Np, D, D)."""
    walk, paths = lineage_paths(problem, x, x0, n, seed, ess_fraction, index)
    w = final_weights(walk.lw)
    return walk.record(second=weighted_second(w, paths), a2=weighted_second(w, np.abs(paths)), **lineage_moments(walk, paths))


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """the restatement of a case of test_particle_filter_cpu.case, computed once per process and shared by the CPU and GPU tests (read-only)"""
    q, x, x0 = case(tag)
    return particle_covariance_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", WALK_TAGS)
def test_same_walk_and_moments_as_the_moments_restatement(tag):
    q, x, x0 = case(tag)
    for start in (None, x0):
        for frac in (0.0, 0.5, 1.0):
            got = particle_covariance_numpy(q, x, start, 17, SEED, frac)
            want = particle_moments_numpy(q, x, start, 17, SEED, frac)
            for key in ("lw", "state", "ancestors", "resampled", "m1", "m2", "lineage_ess", "ess", "a1"):
                assert np.array_equal(got[key], want[key]), (tag, frac, key)
            assert got["margins"] == want["margins"]


@pytest.mark.parametrize("tag", WALK_TAGS + ["l96d40_rk4_p"])
def test_diagonal_and_symmetry(tag):
    """the diagonal of `second` is M2 summed in another association -- (W x) x in place of W x^2, n = 65 non-negative terms each rounded to
    1.2e-16: within 65 * 2.3e-16 < 1e-13 of M2, relatively --, the matrix is symmetric to the bit, and |second| <= a2 entry by entry"""
    q, x, x0 = case(tag)
    ref = particle_covariance_numpy(q, x, None, 65, SEED, 0.5)
    d = ref["m1"].shape[1]
    assert ref["second"].shape == ref["a2"].shape == (int(q.n_pts), d, d)
    assert np.array_equal(ref["second"], np.transpose(ref["second"], (0, 2, 1))) and np.array_equal(ref["a2"], np.transpose(ref["a2"], (0, 2, 1)))
    diag = np.diagonal(ref["second"], axis1=1, axis2=2)
    assert np.all(np.abs(diag - ref["m2"]) <= 1e-13 * ref["m2"])
    assert np.all(np.abs(ref["second"]) <= ref["a2"] * (1.0 + 1e-13))
    if d > 1:      # (a matrix, not a diagonal: off-diagonal entries are there)
        off = ref["second"][:, np.arange(1, d), np.arange(d - 1)]
        assert np.any(np.abs(off) > 0.0)


@pytest.mark.parametrize("tag", ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p", "quiet_l96d17"])
def test_backward_recursion_is_the_forward_algorithm(tag):
    """descendant_weights on the restatement's histories, applied to its clouds, gives at the observation indices the matrices the carried
    paths give; both are sums of at most n products of a weight and two states, each rounded to a few 1e-16: 1e-12 of sum W |x_a| |x_b|
    holds for every n used here"""
    q, x, x0 = case(tag)
    worst = 0.0
    tiny = float(np.finfo(float).tiny)
    for start in (None, x0):
        for n, frac in ((17, 0.5), (65, 1.0), (65, 0.5)):
            ref = particle_covariance_numpy(q, x, start, n, SEED, frac)
            table = descendant_weights(ref["lw"], ref["ancestors"], ref["resampled"])
            for j, t in enumerate(ref["obs_t"]):
                sec = weighted_second(table[j], ref["clouds"][j][:, None, :])[0]
                worst = max(worst, float(np.max(np.abs(sec - ref["second"][t]) / (ref["a2"][t] + tiny))))
    print(tag, "worst backward against forward, relative to sum W |x_a| |x_b|:", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("tag", FIXTURES)
def test_without_resampling_it_is_the_reweighted_stored_paths(tag):
    """ess_fraction = 0: the matrices are the weighted second moments of sample_paths_numpy's paths under path_weights_numpy's weights.
    The two log-weights agree to 1e-12 (1 + scale) (test_particle_filter_cpu asserts it), so the normalised weights agree to twice that,
    relatively, and so do sums of them against the sums of their absolute terms"""
    q, x, x0 = case(tag)
    worst = 0.0
    tiny = float(np.finfo(float).tiny)
    for start in (None, x0):
        ref = particle_covariance_numpy(q, x, start, 9, SEED, 0.0)
        init, path, obs, scale = path_weights_numpy(q, x, start, 9, SEED)
        paths = sample_paths_numpy(q, "posterior", x, start, 9, 1, SEED)
        lw = init + path + obs
        w = np.exp(lw - lw.max())
        w = w / w.sum()
        bound = 2e-12 * (1.0 + float(scale.max())) + 1e-14
        sec, a2 = weighted_second(w, paths), weighted_second(w, np.abs(paths))
        worst = max(worst, float(np.max(np.abs(ref["second"] - sec) / (a2 + tiny))) / bound)
        assert not ref["resampled"].any()
    print(tag, "worst deviation from the reweighted stored paths, in units of its bound:", worst)
    assert worst <= 1.0


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(5, 4, 3)) + 2.0      # 5 slots, 4 kept indices, D = 3
    w = np.array([0.1, 0.2, 0.3, 0.25, 0.15])
    mean, second = np.einsum("i,ikd->kd", w, pts), weighted_second(w, pts)
    rec = SmoothingCovariance([-700.0, -701.0], mean, second, 3, 11, [0, 4, 10], [1.5, 1.6, 1.7, 1.8], [2.0, 1.0, 1.5], [1, 0, 0])
    assert len(rec) == 2 and np.array_equal(rec.grid, [0, 3, 6, 9]) and rec.resampled.dtype == bool
    assert np.array_equal(rec.mean, mean) and np.array_equal(rec.second, second)
    cov = second - mean[:, :, None] * mean[:, None, :]
    assert np.array_equal(rec.cov, cov) and np.array_equal(rec.var, np.diagonal(cov, axis1=1, axis2=2))
    centred = pts - mean[None]
    assert np.allclose(rec.cov, np.einsum("i,ika,ikb->kab", w, centred, centred), rtol=0.0, atol=1e-13)
    sd = np.sqrt(rec.var)
    assert np.allclose(rec.corr, cov / (sd[:, :, None] * sd[:, None, :]), rtol=1e-14) and np.allclose(np.diagonal(rec.corr, axis1=1, axis2=2), 1.0)
    assert np.all(np.abs(rec.corr) <= 1.0 + 1e-12)
    # index 0 lies in stretch 0 (k <= t_0 = 0), 3 in stretch 1 (0 < k <= 4), 6 and 9 in stretch 2 (4 < k <= 10)
    assert np.array_equal(rec.lineage_ess_on_grid(), [1.5, 1.6, 1.7, 1.7])
    assert np.isclose(rec.log_evidence(), -700.0 + np.log((1.0 + np.exp(-1.0)) / 2.0))
    m6, c6 = rec.gaussian(6)      # a kept index
    assert np.array_equal(m6, mean[2]) and np.array_equal(c6, cov[2])
    for k in (4, 10, 12, -3):     # not kept: off the stride, behind the grid, before it
        with pytest.raises(ValueError):
            rec.gaussian(k)
    last = SmoothingCovariance([0.0], mean[:3], second[:3], 5, 11, [], [1.0])      # grid 0, 5, 10: the last grid index is kept
    assert np.array_equal(last.gaussian(10)[0], mean[2]) and np.array_equal(last.gaussian(10)[1], cov[2])
    one = SmoothingCovariance([0.0], mean[:, :1], second[:, :1, :1], 3, 11, [], [1.0], single_dim=True)
    assert one.mean.shape == one.second.shape == one.cov.shape == one.var.shape == one.corr.shape == (4,)
    assert np.ndim(one.gaussian(3)[0]) == 0 and np.ndim(one.gaussian(3)[1]) == 0 and np.array_equal(one.lineage_ess_on_grid(), np.ones(4))
    neg = SmoothingCovariance([0.0], np.array([[1.0]]), np.array([[[1.0 - 1e-16]]]), 5, 3, [], [1.0])
    assert neg.cov[0, 0, 0] < 0.0 and neg.var[0, 0] < 0.0 and np.isnan(neg.corr[0, 0, 0])      # (as it comes: not clipped)
    for bad in (lambda: SmoothingCovariance([], mean, second, 3, 11, [], [1.0]), lambda: SmoothingCovariance([0.0], mean, second, 2, 11, [], [1.0]),
                lambda: SmoothingCovariance([0.0], mean, second, 0, 11, [], [1.0]), lambda: SmoothingCovariance([0.0], mean, second, 3, 11, [1, 2], [1.0]),
                lambda: SmoothingCovariance([0.0], mean, second[:, :2], 3, 11, [], [1.0]),
                lambda: SmoothingCovariance([0.0], mean, second, 3, 11, [], [1.0], [1.0], [])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_covariance" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_covariance\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed, "
                    "double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, "
                    "double* mean, double* second, double* lineage_ess_or_null, double* ess_or_null, int32_t* resampled_or_null")
    lib = va.load()
    assert hasattr(lib, "vgpa_particle_covariance"), "declared and not exported by the built library"
    assert len(lib.vgpa_particle_covariance.argtypes) == 16


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0", "prior"]),
                          (va.VarGP, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"]),
                          (va.ProblemBatch, ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"])]:
        fn = getattr(owner, "particle_covariance", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["stride"].default == 1
    assert va.SmoothingCovariance is SmoothingCovariance and "SmoothingCovariance" in va.__all__
    for name in ("mean", "second", "cov", "var", "corr", "grid"):
        assert isinstance(getattr(SmoothingCovariance, name), property), name
    for name in ("lineage_ess_on_grid", "log_evidence", "gaussian"):
        assert callable(getattr(SmoothingCovariance, name))
