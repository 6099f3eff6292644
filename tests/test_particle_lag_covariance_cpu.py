"""
The two-time moments of the particle smoother (vgpa_particle_lag_covariance, vgpa_path_cross_moments) without a device:
the restatement, its floor, the runs of tests/test_particle_lag_covariance.py (GPU), the record SmoothingLagCovariance and the host-side
surface.  The GPU module imports everything from here and only runs the device and compares.

The restatement.  lag_cross_numpy(paths, W, anchor_rows, dtype): with paths (n, n_keep, D) and weights W (n,)
    mean[k][a]        = sum_i W_i x_i(k)[a]
    cross[q][k][a][b] = sum_i (W_i x_i(r_q)[b]) x_i(k)[a]
the terms formed as the kernels form them (the weight on the anchor's side) and added as a balanced tree (extended_ref._sum), in float64 or
in longdouble.  W comes from log-weights (extended_ref.normalised_weights, in the same dtype) or is used as given.

The floor, by the counting rule of test_particle_rounding_cpu.py (every rounding of a careful evaluation once, a sum of n terms as a tree
of levels(n) additions per term), 2^-53 times
    size = sum_i W_i (2 + |lw_i - max lw| + 2 levels(n)) |x_i(k)[a]| |x_i(s)[b]|
-- the "sum W v" size of that module with one more product.  With weights given as they are the |lw - max lw| term drops (the weights
carry no rounding of their own), and the mean's size is that module's sum W v itself.

Measured here, numpy in the device's place (float64, added one term at a time and as a tree) against the longdouble restatement:
n in {1, 17, 65, 300}, weight spreads 3 and 700: within one floor in both orders (asserted; worst of the tree-added runs 0.53).  On the runs of the GPU module (the restated
trajectories of test_particle_paths_cpu.reference) the tree-added float64 restatement stays within one floor on every run (asserted); added
one path at a time it reaches 1.07 floors at n = 300 -- 300 sequential additions are not the 2 levels(n) = 18 the floor counts -- and is held
to the GPU module's bound, 32 max(e_o, 1), instead.

The mutants (test_mutants prints each factor over the right-hand side 32 max(e_o, 1) of the GPU module's bound):
  a weight paired with the neighbouring path, (a, b) transposed, the anchor row off by one kept index   over by >= 1e6
  weights normalised by S (1 + 2^-30)                                                                    over by >= 1e2
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.lagcov import LagCovariance
from vgpa_amd.particles import ParticleFilterResult, SmoothingLagCovariance
from conftest import ROOT
from test_particle_api_cpu import B, D, HANDLE, LEN_X, M, N, N_KEEP, NP, PRIOR, SEED as API_SEED, STRIDE, ESS_FRACTION, X, X0, prototype
from test_particle_filter_cpu import QUIET
from test_particle_paths_cpu import reference
from test_particle_rounding_cpu import FACTOR, UNIT, errors, floor_covers_the_oracle, record, within
from test_path_weights_cpu import TAGS

LD, F64 = np.longdouble, np.float64
WORST = {}

# The runs of the GPU module: (tag, start, particles, ess_fraction, stride).  D = 1, 1, 3, 12, 17, 40, 4, 5, 64 (TAGS: the lane kernel at
# 1, 3 and 4, NT = 16, 16, 32, 48, 64 above; 12 and 17 odd against the tile, 64 = NT); one path, a partial group of four (17, 65), one
# block of 64 and one path, several blocks; every grid index and every fourth (n_keep = 41 and 11 at the 41-point grids: neither a multiple
# of the four kept rows a workgroup takes)
SIZES = (1, 17, 65, 300)
RUNS = [(t, "given" if i % 2 else "drawn", n, 0.5 if n != 65 else 1.0, 4 if n == 300 else 1) for i, t in enumerate(TAGS) for n in SIZES] + \
       [(t, "given", 65, 0.5, 4) for t in QUIET]


def anchors_of(n_pts, stride, obs_t):
    """three anchors on the kept grid: index 0, an observation index where one is kept (else the middle), the last kept index"""
    last = (n_pts - 1) // stride * stride
    kept_obs = [int(t) for t in np.asarray(obs_t).ravel() if 0 < int(t) < last and int(t) % stride == 0]
    mid = kept_obs[len(kept_obs) // 2] if kept_obs else (last // stride // 2) * stride
    return np.array(sorted({0, mid, last}), dtype=np.int64)


def _add(terms, order):
    if order == "tree":
        return xr._sum(terms, 0)
    acc = np.zeros(terms.shape[1:], dtype=terms.dtype)
    for t in terms:      # one term at a time, in increasing path index
        acc = acc + t
    return acc


def lag_cross_numpy(paths, W, anchor_rows, dtype, log_w=None, order="tree", total_scale=None):
    """(mean (n_keep, D), cross (n_anchor, n_keep, D, D), size of mean, size of cross) in `dtype`; W (n,) as given, or None with log_w (n,).
    The sizes are in units of 2^-53 (the head of the file)."""
    T = dtype
    x = np.asarray(paths, dtype=T)
    n, n_keep, d = x.shape
    if log_w is not None:
        w, own = xr.normalised_weights(log_w, T, total_scale)
    else:
        w, own = np.asarray(W, dtype=T).ravel(), np.ones(n, dtype=T)      # (own: a weight's roundings and its product with x, in units of the term)
    lev = 2 * xr.levels(n)
    ax = np.abs(x)
    mean = _add(w[:, None, None] * x, order)
    size_mean = _add((w * (own + lev))[:, None, None] * ax, order)
    rows = np.asarray(anchor_rows, dtype=np.int64).ravel()
    cross, size = np.empty((rows.size, n_keep, d, d), dtype=T), np.empty((rows.size, n_keep, d, d), dtype=T)
    step = max(1, 2 ** 21 // (n * d * d))      # (a few kept indices at a time: 300 paths at D = 64 would not fit at once)
    for q, r in enumerate(rows):
        wb, sb = w[:, None] * x[:, r], (w * (own + 1 + lev))[:, None] * ax[:, r]
        for k0 in range(0, n_keep, step):
            cross[q, k0:k0 + step] = _add(wb[:, None, None, :] * x[:, k0:k0 + step, :, None], order)
            size[q, k0:k0 + step] = _add(sb[:, None, None, :] * ax[:, k0:k0 + step, :, None], order)
    return mean, cross, size_mean, size


def _own_term_check():
    """the size's weight factor: 2 + |lw - max lw| + 2 levels(n) from log-weights (normalised_weights' 1 + |lw - max lw| and one more
    product), 2 + 2 levels(n) with weights as given"""
    lw = np.array([0.0, -3.0])
    _, _, sm, sc = lag_cross_numpy(np.ones((2, 1, 1)), None, [0], F64, log_w=lw)
    w = np.exp(lw) / np.sum(np.exp(lw))
    assert np.isclose(sc[0, 0, 0, 0], w[0] * (2 + 0 + 2) + w[1] * (2 + 3 + 2)) and np.isclose(sm[0, 0], w[0] * (1 + 0 + 2) + w[1] * (1 + 3 + 2))
    _, _, sm, sc = lag_cross_numpy(np.ones((2, 1, 1)), [0.25, 0.75], [0], F64)
    assert np.isclose(sc[0, 0, 0, 0], 2 + 2) and np.isclose(sm[0, 0], 1 + 2)


def test_the_size_is_the_one_stated():
    _own_term_check()


def compare(worst, label, family, got_mean, got_cross, paths, anchor_rows, log_w=None, W=None):
    """the failures of mean and cross against the longdouble restatement on `paths`, in floors; the float64 restatement is the oracle"""
    m_x, c_x, s_m, s_c = lag_cross_numpy(paths, W, anchor_rows, LD, log_w=log_w)
    m_o, c_o, _, _ = lag_cross_numpy(paths, W, anchor_rows, F64, log_w=log_w)
    return (record(worst, family, "sum W x(k)", label, got_mean, m_x, m_o, s_m) +
            record(worst, family, "sum W x(k) x(s)^T", label, got_cross, c_x, c_o, s_c))


def synthetic(n, spread, d=3, n_keep=5, seed=0):
    rng = np.random.default_rng([n, spread, seed])
    paths = rng.standard_normal((n, n_keep, d)) * np.exp(rng.uniform(-2, 2, (1, 1, d))) + rng.uniform(-3, 3, (1, n_keep, d))
    lw = -spread * rng.uniform(0, 1, n)
    lw[rng.integers(n)] = -float(spread)
    return paths, lw


@pytest.mark.parametrize("spread", [3, 700])
@pytest.mark.parametrize("n", SIZES)
def test_floor_covers_the_oracle(n, spread):
    """numpy in the device's place, adding as a tree and one term at a time, weights from log-weights and as given"""
    paths, lw = synthetic(n, spread)
    rows = [0, 2, 4]
    with floor_covers_the_oracle():
        for order in ("tree", "one at a time"):
            m, c, _, _ = lag_cross_numpy(paths, None, rows, F64, log_w=lw, order=order)
            assert not compare(WORST, f"n={n} spread {spread} {order}", "numpy", m, c, paths, rows, log_w=lw)
            w = xr.normalised_weights(lw, F64)[0]
            m, c, _, _ = lag_cross_numpy(paths, w, rows, F64, order=order)
            assert not compare(WORST, f"n={n} spread {spread} {order} given weights", "numpy", m, c, paths, rows, W=w)


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "-".join(map(str, r)))
def test_floor_covers_the_oracle_on_the_gpu_runs(run):
    """every run of the GPU module, on the restated trajectories: the float64 restatement (added as a tree, the evaluation the floor counts)
    within one floor; added one path at a time, the kernels' order, within the GPU module's bound -- that order is no careful evaluation of
    300 terms and stands at up to 1.07 floors (l63_euler_p, n = 300), which is printed and not held to 1"""
    tag, start, n, frac, stride = run
    want = reference(tag, start, n, frac)
    paths = want["paths"][:, ::stride]
    rows = anchors_of(want["paths"].shape[1], stride, want["obs_t"]) // stride
    with floor_covers_the_oracle():
        m, c, _, _ = lag_cross_numpy(paths, None, rows, F64, log_w=want["lw"])
        assert not compare(WORST, "-".join(map(str, run)), "numpy", m, c, paths, rows, log_w=want["lw"])
    m, c, _, _ = lag_cross_numpy(paths, None, rows, F64, log_w=want["lw"], order="one at a time")
    assert not compare(WORST, "-".join(map(str, run)) + " one at a time", "numpy, one at a time", m, c, paths, rows, log_w=want["lw"])


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d5", "l96d12_euler_p"])
def test_lineages_at_the_observations(tag):
    """ParticleFilterResult.lineages() -- the clouds traced through the ancestors -- contracted with log_w is the restatement on the
    trajectories' rows at the observation indices"""
    want = reference(tag, "drawn", 65, 0.5)
    assert want["resampled"].any()
    rec = ParticleFilterResult(want["lw"], want["state"], want["ess"], want["resampled"], want["ancestors"], want["clouds"])
    lin, at_obs = rec.lineages(), want["paths"][:, want["obs_t"]]
    rows = np.arange(at_obs.shape[1])
    m, c, _, _ = lag_cross_numpy(lin, None, rows, F64, log_w=rec.log_w)
    assert not compare(WORST, tag + " lineages()", "numpy", m, c, at_obs, rows, log_w=want["lw"])


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d5", "l96d12_euler_p"])
def test_own_index_is_the_smoothing_second_moment(tag):
    """At an anchor's own kept index the cross moment and test_particle_rounding_cpu.check_smoothing's sum W x x^T (extended_ref.weighted_sum on
    the products) are two evaluations of one sum: their float64 values differ by no more than the plain sum of the two floors.  (The GPU
    module holds the device's cross and second to 32 times that sum.)"""
    want = reference(tag, "given", 65, 0.5)
    paths, lw = want["paths"], want["lw"]
    rows = anchors_of(paths.shape[1], 1, want["obs_t"])
    _, c, _, size = lag_cross_numpy(paths, None, rows, F64, log_w=lw, order="one at a time")
    for q, r in enumerate(rows):
        sq = np.einsum("na,nb->nab", paths[:, r], paths[:, r])
        second, size2 = xr.weighted_sum(lw, sq, F64)
        assert np.all(np.abs(c[q, r] - second) <= UNIT * (size[q, r] + size2)), (tag, r)


MUT = 1.0 + 2.0 ** -30


def test_mutants():
    """the floor rejects each mutant, by the factor stated at the head of the file, on every synthetic case with more than one path"""
    for n in SIZES[1:]:
        for spread in (3, 700):
            paths, lw = synthetic(n, spread)
            rows = np.array([1, 3])
            m_x, c_x, s_m, s_c = lag_cross_numpy(paths, None, rows, LD, log_w=lw)
            _, c_o, _, _ = lag_cross_numpy(paths, None, rows, F64, log_w=lw)
            w = xr.normalised_weights(lw, F64)[0]
            mutants = {
                "neighbouring weight": (lag_cross_numpy(paths, np.roll(w, 1), rows, F64)[1], 1e6),
                "(a, b) transposed": (np.swapaxes(c_o, -1, -2), 1e6),
                "anchor row off by one": (lag_cross_numpy(paths, None, rows + 1, F64, log_w=lw)[1], 1e6),
                "S (1 + 2^-30)": (lag_cross_numpy(paths, None, rows, F64, log_w=lw, total_scale=MUT)[1], 1e2),
            }
            for name, (c_m, factor) in mutants.items():
                e_k, e_o = errors(c_m, c_x, c_o, s_c)
                over = e_k / (FACTOR * max(e_o, 1.0))
                print(f"n={n} spread {spread} mutant {name}: e_k={e_k:.3g} floors, over the bound by {over:.3g}")
                assert not within(e_k, e_o) and over >= factor, (name, n, spread, over)


# ---- the record ------------------------------------------------------------------------------------------------------------------------------
def _hand_made(d=2, n=5, n_pts=13, stride=3, seed=3):
    rng = np.random.default_rng(seed)
    n_keep = (n_pts - 1) // stride + 1
    paths = rng.standard_normal((n, n_keep, d)) + np.arange(n_keep)[None, :, None]
    lw = rng.standard_normal(n)
    w = np.exp(lw - lw.max()) / np.sum(np.exp(lw - lw.max()))
    anchors = np.array([0, 6, 12])
    mean = np.einsum("i,ika->ka", w, paths)
    cross = np.einsum("i,ika,iqb->qkab", w, paths, paths[:, anchors // stride])
    return paths, lw, w, anchors, mean, cross


def test_record_on_a_hand_made_table():
    paths, lw, w, anchors, mean, cross = _hand_made()
    rec = SmoothingLagCovariance(lw, mean, cross, anchors, 3, 13, [4, 9], [5.0, 3.0, 2.0], [4.0, 3.0], [1, 0])
    assert np.array_equal(rec.mean, mean) and np.array_equal(rec.cross, cross) and np.array_equal(rec.anchors, anchors)
    assert np.array_equal(rec.lineage_ess, [5.0, 3.0, 2.0]) and np.array_equal(rec.grid, [0, 3, 6, 9, 12]) and len(rec) == 5
    assert np.array_equal(rec.lineage_ess_on_grid(), [5.0, 5.0, 3.0, 3.0, 2.0])
    dev = paths - mean[None]
    centred = lambda k, s: np.einsum("i,ia,ib->ab", w, dev[:, k // 3], dev[:, s // 3])      # noqa: E731
    for k in (0, 3, 6, 9, 12):
        for s in anchors:
            assert np.allclose(rec.cov(k, s), centred(k, s), rtol=0, atol=1e-13) and np.array_equal(rec.cov(k, s), cross[list(anchors).index(s), k // 3] - np.outer(mean[k // 3], mean[s // 3]))
    assert np.array_equal(rec.cov(6, 9), rec.cov(9, 6).T) and np.array_equal(rec.cov(9, 6), cross[1, 3] - np.outer(mean[3], mean[2]))
    with pytest.raises(KeyError):
        rec.cov(3, 9)      # neither is an anchor
    with pytest.raises(KeyError):
        rec.cov(4, 6)      # not kept
    sd = lambda k: np.sqrt(np.diag(centred(k, k)))      # noqa: E731
    assert np.allclose(rec.corr(12, 6), centred(12, 6) / np.outer(sd(12), sd(6)), rtol=1e-12)
    assert np.allclose(np.diag(rec.corr(6, 6)), 1.0, rtol=1e-12)
    inc = np.einsum("i,ia,ib->ab", w, dev[:, 4] - dev[:, 2], dev[:, 4] - dev[:, 2])
    assert np.allclose(rec.increment_var(12, 6), inc, rtol=0, atol=1e-12)
    st = np.stack([centred(k, k) for k in (0, 3, 6, 9, 12)])
    assert np.allclose(rec.increment_var(9, 6, st), np.einsum("i,ia,ib->ab", w, dev[:, 3] - dev[:, 2], dev[:, 3] - dev[:, 2]), rtol=0, atol=1e-12)
    assert np.array_equal(rec.marginal(9, st), st[3]) and np.array_equal(rec.marginal(6), rec.cov(6, 6))
    var = np.diagonal(st, axis1=1, axis2=2)
    auto = rec.autocorrelation(6, var)
    assert auto.shape == (5, 2) and np.allclose(auto[2], 1.0, rtol=1e-12)
    assert np.allclose(auto[4], np.diag(centred(12, 6)) / (sd(12) * sd(6)), rtol=1e-12)
    bare = rec.autocorrelation(6)
    assert np.allclose(bare[[0, 2, 4]], auto[[0, 2, 4]], rtol=1e-12) and np.all(np.isnan(bare[[1, 3]]))
    with pytest.raises(KeyError):
        rec.autocorrelation(3)
    m, c = rec.joint()
    assert m.shape == (6,) and c.shape == (6, 6) and np.array_equal(c, c.T) and np.array_equal(m, mean[[0, 2, 4]].ravel())
    by_hand = np.block([[centred(si, sj) for sj in anchors] for si in anchors])
    assert np.allclose(c, by_hand, rtol=0, atol=1e-12)
    for i, si in enumerate(anchors):
        for j, sj in enumerate(anchors[:i]):
            assert np.array_equal(c[2 * i:2 * i + 2, 2 * j:2 * j + 2], rec.cov(si, sj))
    assert np.all(np.linalg.eigvalsh(c) > -1e-12)


def test_record_of_a_one_dimensional_model_and_a_negative_variance():
    paths, lw, w, anchors, mean, cross = _hand_made(d=1)
    rec = SmoothingLagCovariance(lw, mean, cross, anchors, 3, 13, [4, 9], [5.0, 3.0, 2.0], single_dim=True)
    assert rec.mean.shape == (5,) and rec.cross.shape == (3, 5) and np.ndim(rec.cov(9, 6)) == 0 and np.ndim(rec.corr(12, 6)) == 0
    assert np.ndim(rec.increment_var(12, 0)) == 0 and rec.autocorrelation(6).shape == (5,)
    m, c = rec.joint()
    assert m.shape == (3,) and c.shape == (3, 3) and np.array_equal(c, c.T)
    # one lineage: second - mean^2 is rounding noise of either sign; a negative one stays negative, and its correlations are nan
    one = np.array([0.1, 0.7])
    raw = np.outer(one, one)                      # [anchor][kept index]: one lineage, cross = mean mean^T
    raw[0, 0] = np.nextafter(raw[0, 0], 0.0)      # ... but for one rounding
    neg = SmoothingLagCovariance([0.0], one[:, None], raw[:, :, None, None], [0, 3], 3, 4, [], [1.0], single_dim=True)
    assert neg.cov(0, 0) < 0.0 and neg.cov(3, 0) == 0.0 and neg.increment_var(3, 0) < 0.0
    assert np.isnan(neg.corr(3, 0)) and np.isnan(neg.autocorrelation(3)[0])


REFUSED = [
    (lambda: SmoothingLagCovariance([], np.zeros((5, 2)), np.zeros((1, 5, 2, 2)), [0], 3, 13, [], [1.0]), " SmoothingLagCovariance: at least one particle."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((1, 5, 2, 2)), [0], 0, 13, [], [1.0]), " SmoothingLagCovariance: stride and n_pts must be at least 1."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((4, 2)), np.zeros((1, 5, 2, 2)), [0], 3, 13, [], [1.0]),
     " SmoothingLagCovariance: mean must be (n_keep, D) and cross (n_anchor, n_keep, D, D)."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((2, 5, 2, 2)), [0], 3, 13, [], [1.0]),
     " SmoothingLagCovariance: mean must be (n_keep, D) and cross (n_anchor, n_keep, D, D)."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((2, 5, 2, 2)), [6, 3], 3, 13, [], [1.0]),
     " SmoothingLagCovariance: anchors must be strictly increasing kept grid indices."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((1, 5, 2, 2)), [4], 3, 13, [], [1.0]),
     " SmoothingLagCovariance: anchors must be strictly increasing kept grid indices."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((1, 5, 2, 2)), [15], 3, 13, [], [1.0]),
     " SmoothingLagCovariance: anchors must be strictly increasing kept grid indices."),
    (lambda: SmoothingLagCovariance([0.0], np.zeros((5, 2)), np.zeros((1, 5, 2, 2)), [3], 3, 13, [4], [1.0]),
     " SmoothingLagCovariance: obs_t, lineage_ess, ess and resampled do not belong together."),
]


@pytest.mark.parametrize("i", range(len(REFUSED)))
def test_record_refuses_by_text(i):
    make, text = REFUSED[i]
    with pytest.raises(ValueError) as err:
        make()
    assert str(err.value) == text


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("vgpa_particle_lag_covariance", "vgpa_path_cross_moments")


def test_symbols_and_prototypes():
    header = open(os.path.join(ROOT, "include", "vgpa_hip.h")).read()
    lib = va.load()
    for entry in ENTRIES:
        assert entry in _lib.SYMBOLS and re.search(r"\bint\s+" + entry + r"\s*\(", header) and hasattr(lib, entry)
        assert len(getattr(lib, entry).argtypes) == len(prototype(entry))
    names = [n for n, _ in prototype("vgpa_particle_lag_covariance")]
    assert names == ["ctx", "x", "x0", "n_paths", "stride", "seed", "ess_fraction", "prior_mu", "prior_tau", "n_anchor", "anchors", "logw", "state",
                     "mean", "cross", "lineage_ess", "ess", "resampled"]
    assert [n for n, _ in prototype("vgpa_path_cross_moments")] == ["ctx", "paths", "weights", "n_paths", "n_keep", "n_anchor", "anchor_rows", "mean", "cross"]


def test_python_surface():
    for cls in (va.VarGP, va.ProblemBatch):
        assert list(inspect.signature(cls.particle_kernel).parameters)[:4] == ["self", "n_paths", "seed", "anchors"]
    sig = inspect.signature(va.Context.particle_lag_covariance)
    assert list(sig.parameters) == ["self", "n_paths", "seed", "anchors", "stride", "ess_fraction", "x", "x0", "prior"]
    assert list(inspect.signature(va.Context.path_cross_moments).parameters) == ["self", "paths", "anchor_rows", "weights"]
    assert va.SmoothingLagCovariance is SmoothingLagCovariance and "SmoothingLagCovariance" in va.__all__
    assert hasattr(va.SmoothingPaths, "lag_covariance")
    for name in ("cov", "corr", "increment_var", "joint", "marginal"):      # named and called as LagCovariance's
        ours, theirs = getattr(SmoothingLagCovariance, name), getattr(LagCovariance, name)
        assert list(inspect.signature(ours).parameters) == list(inspect.signature(theirs).parameters), name


class _Recorder:
    """stands in for the ctypes handle: records the arguments, reads the input arrays while they are alive, returns 0"""

    def __init__(self, inputs):
        self.calls, self.inputs = [], inputs

    def __getattr__(self, entry):
        def call(*args):
            seen = {}
            for (name, _), arg in zip(prototype(entry), args):
                if name in self.inputs and arg is not None:
                    dtype, count = self.inputs[name]
                    seen[name] = np.frombuffer(ctypes.string_at(arg.value, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
            self.calls.append((entry, args, seen))
            return 0
        return call


def _bare_context(inputs):
    c = object.__new__(va.Context)
    c._lib, c._h = _Recorder(inputs), HANDLE
    c.B, c.D, c.Np, c.n_obs, c.len_x = B, D, NP, M, LEN_X
    return c


def _check_kinds(entry, args):
    params, argtypes = prototype(entry), getattr(va.load(), entry).argtypes
    assert len(args) == len(argtypes) == len(params) and args[0] is HANDLE
    at = {}
    for (name, kind), argtype, arg in zip(params, argtypes, args):
        at[name] = arg
        if kind == "ptr":
            assert argtype is ctypes.c_void_p and (arg is None or (isinstance(arg, ctypes.c_void_p) and arg.value)), name
        elif kind == "f64":
            assert argtype is ctypes.c_double and type(arg) is float, name
        elif kind == "u64":
            assert argtype is ctypes.c_uint64 and type(arg) is int and 0 <= arg < 2 ** 64, name
        else:
            assert argtype in (ctypes.c_int32, ctypes.c_int) and type(arg) is int and -2 ** 31 <= arg < 2 ** 31, name
    return at


def test_call_layout_of_the_fused_entry():
    anchors = [0, 3, 9]
    ins = {"x": (F64, B * LEN_X), "x0": (F64, B * D), "prior_mu": (F64, B * D), "prior_tau": (F64, B * D * D), "anchors": (np.int64, 3)}
    c = _bare_context(ins)
    res = c.particle_lag_covariance(N, API_SEED, anchors, stride=STRIDE, ess_fraction=ESS_FRACTION, x=X, x0=X0, prior=PRIOR)
    assert [e for e, _, _ in c._lib.calls] == ["vgpa_particle_lag_covariance"]
    _, args, seen = c._lib.calls[0]
    at = _check_kinds("vgpa_particle_lag_covariance", args)
    assert (at["n_paths"], at["stride"], at["seed"], at["ess_fraction"], at["n_anchor"]) == (N, STRIDE, API_SEED, ESS_FRACTION, 3)
    for name, value in {"x": X, "x0": X0, "prior_mu": PRIOR[0], "prior_tau": PRIOR[1], "anchors": anchors}.items():
        assert np.array_equal(seen[name], np.asarray(value).ravel()), name
    outs = {"logw": ("log_w", (B, N), None), "state": ("state", (B, N, D), None), "mean": ("mean", (B, N_KEEP, D), None),
            "cross": ("cross", (B, 3, N_KEEP, D, D), None), "lineage_ess": ("lineage_ess", (B, M + 1), 0.0), "ess": ("ess", (B, M), 0.0)}
    for name, (key, shape, fill) in outs.items():
        assert at[name].value == res[key].ctypes.data and res[key].shape == shape and res[key].dtype == F64 and res[key].flags["C_CONTIGUOUS"], name
        assert fill is None or np.all(res[key] == fill), name
    assert at["resampled"].value == res["resampled"].ctypes.data and res["resampled"].dtype == np.int32
    assert list(res) == ["log_w", "state", "ess", "resampled", "mean", "cross", "lineage_ess"]
    bare = _bare_context(ins)
    bare.particle_lag_covariance(N, API_SEED, 6)      # one anchor as a scalar; nothing else given
    at = _check_kinds("vgpa_particle_lag_covariance", bare._lib.calls[0][1])
    assert at["n_anchor"] == 1 and at["stride"] == 1 and all(at[k] is None for k in ("x", "x0", "prior_mu", "prior_tau"))
    for bad, text in (([0.5], "anchors must be a 1-D sequence of integers"), ([[0, 1]], "anchors must be a 1-D sequence of integers"),
                      ([2 ** 63], "anchors must fit into 64 bits")):
        with pytest.raises(ValueError, match=re.escape(text)):
            bare.particle_lag_covariance(N, 1, bad)
    assert len(bare._lib.calls) == 1


def test_call_layout_of_the_operator():
    rng = np.random.default_rng(5)
    paths, weights, rows = rng.standard_normal((B, N, N_KEEP, D)), rng.uniform(0, 1, (B, N)), [3, 0, 3]
    ins = {"paths": (F64, paths.size), "weights": (F64, weights.size), "anchor_rows": (np.int32, 3)}
    c = _bare_context(ins)
    mean, cross = c.path_cross_moments(paths, rows, weights=weights)
    _, args, seen = c._lib.calls[0]
    at = _check_kinds("vgpa_path_cross_moments", args)
    assert (at["n_paths"], at["n_keep"], at["n_anchor"]) == (N, N_KEEP, 3)
    assert np.array_equal(seen["paths"], paths.ravel()) and np.array_equal(seen["weights"], weights.ravel()) and np.array_equal(seen["anchor_rows"], rows)
    assert at["mean"].value == mean.ctypes.data and at["cross"].value == cross.ctypes.data
    assert mean.shape == (B, N_KEEP, D) and cross.shape == (B, 3, N_KEEP, D, D) and mean.dtype == cross.dtype == F64
    c.path_cross_moments(paths, 1)
    at = _check_kinds("vgpa_path_cross_moments", c._lib.calls[1][1])
    assert at["weights"] is None and at["n_anchor"] == 1
    for call, text in ((lambda: c.path_cross_moments(paths[0], rows), "paths has shape"), (lambda: c.path_cross_moments(paths[..., :2], rows), "paths has shape"),
                       (lambda: c.path_cross_moments(paths, rows, weights=weights[:, 1:]), "weights has"),
                       (lambda: c.path_cross_moments(paths, [0.5]), "anchor_rows must be a 1-D sequence of integers"),
                       (lambda: c.path_cross_moments(paths, [2 ** 31]), "anchor_rows must fit into 32 bits")):
        with pytest.raises(ValueError, match=re.escape(text)):
            call()
    assert len(c._lib.calls) == 2


def test_print_worst():
    for key, val in sorted(WORST.items()):
        print(key, f"worst e_k / max(e_o, 1) = {val:.3f}")
