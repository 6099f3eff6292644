"""
The smoothing marginals on the grid under the particle filter's genealogy (vgpa_particle_marginals): the numpy restatement, its checks
against the filter and the moments restatement it rides on, the backward integer recursion, the exact smoother of a linear chain, the
mutants of the restatement, the ladders and the conditions on the cases of tests/test_particle_marginals.py, the record SmoothingMarginals
and the host-side surface.

The restatement rides on test_particle_moments_cpu.particle_moments_numpy, in which every slot carries its whole path: its filter (log-weights,
ancestors, decisions) is taken as it is, and the path of the lineage that ends in each final slot -- what that restatement carries and
reduces but does not return -- is walked once more from its ancestors (test_particle_paths_cpu.trace_slots, rewalk_numpy).  That these
are the carried paths to the bit is asserted on every call: their weighted sums are particle_moments_numpy's m1 and m2, array_equal.  Then
    q_i = trunc(W_i 2^62),   bin(x) = #{l: c_l < x},   mass[k'][d][b] = sum_i q_i 1[bin(path_i(k' stride)[d]) = b]
in uint64 (the forward algorithm).  The device computes the same integers the other way round -- the q pushed backwards through the
ancestors, every slot's own visited state binned --; that the two agree exactly is asserted in test_restatement.

Ladders.  Per case and component the L levels are the quantiles 10 % ... 90 % (L = 1: the median) of the sorted distinct visited values,
linearly interpolated: strictly increasing, and wide enough in the middle of the component's range that the surviving lineages of every
case fall into at least two bins at some grid index (asserted below for every case the GPU file runs and every L).  One level at the
median does not split the lineages of every case; where it does not, the level of one component is moved to the midpoint of the widest
gap between two surviving lineages' states at one grid index (splitting_level).
"""
import ctypes
import functools
import inspect
import os
import re

import numpy as np
import pytest
from scipy.special import ndtr

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import SmoothingMarginals, gaussian_ladder
from conftest import ROOT
from test_particle_api_cpu import (B, D, ESS_FRACTION, HANDLE, LEN_X, M, N, N_KEEP, NP, PRIOR, SEED as API_SEED, STRIDE, X, X0, prototype)
from test_particle_events_cpu import SAMPLE, _built, family, gpu_cases, walk_numpy
from test_particle_filter_cpu import case, particle_filter_numpy
from test_particle_moments_cpu import particle_moments_numpy, rts_marginals
from test_particle_paths_cpu import rewalk_numpy, trace_slots

LEVEL_COUNTS = (1, 7, 63)
MUTANTS = ("le", "final_weights", "no_gather", "drop_last", "stride_cursor")      # (and "other_ladder", which needs a batch)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def quantise(lw):
    """q (n,) uint64 = trunc(W 2^62), W = w / sum w with w = exp(lw - max lw): the product by a power of two is exact, the conversion truncates"""
    w = np.exp(lw - lw.max())
    w = w / w.sum()
    return np.floor(w * 2.0 ** 62).astype(np.uint64)


def bins_of(values, ladder, rule="lt"):
    """#{l: c_l < x} of every entry of values (..., D) on the ladders (D, L): compares alone (searchsorted on a sorted ladder counts them); a NaN
    compares false everywhere.  rule "le": the mutant #{l: c_l <= x}"""
    values = np.asarray(values, dtype=float)
    out = np.empty(values.shape, dtype=np.int64)
    for j in range(values.shape[-1]):
        out[..., j] = np.searchsorted(ladder[j], values[..., j], side="left" if rule == "lt" else "right")
    return np.where(np.isnan(values), 0, out)


def add_mass(mass, bins, weights):
    """mass (n_keep, D, L + 1) uint64 += weights (n, n_keep) (or (n,)) at bins (n, n_keep, D), in integer arithmetic"""
    n_keep, d, nb = mass.shape
    idx = (np.arange(n_keep)[None, :, None] * d + np.arange(d)[None, None, :]) * nb + bins
    wide = np.broadcast_to(np.asarray(weights, dtype=np.uint64).reshape(bins.shape[0], -1, 1), bins.shape)
    np.add.at(mass.reshape(-1), idx.ravel(), wide.ravel())
    return mass


def mass_of_paths(paths, q, ladder, stride=1):
    """(n_keep, D, L + 1) uint64: the histogram of whole lineage paths (n, Np, D) at the kept grid indices, path i weighted by q_i"""
    kept = paths[:, ::stride]
    mass = np.zeros((kept.shape[1], kept.shape[2], ladder.shape[1] + 1), dtype=np.uint64)
    return add_mass(mass, bins_of(kept, ladder), q)


def integer_descendant_weights(q, ancestors, resampled):
    """(M + 1, n) uint64: row M = q; row j = row j + 1 where the cloud was carried on at observation j, else Q^j_a = sum of Q^{j+1}_i over the
    slots i with ancestors[j, i] = a, in 64-bit integer arithmetic"""
    flags = np.asarray(resampled).astype(bool).ravel()
    out = np.zeros((flags.size + 1, q.size), dtype=np.uint64)
    out[-1] = q
    for j in range(flags.size - 1, -1, -1):
        if flags[j]:
            np.add.at(out[j], np.asarray(ancestors[j], dtype=np.int64), out[j + 1])
        else:
            out[j] = out[j + 1]
    return out


def mass_backward(walk, ladder, stride=1, mutant=None, other_ladder=None):
    """The device's way round, from test_particle_events_cpu.walk_numpy's record: every slot's own visited state x_i(k) binned with the integer
    descendant weight Q^{j(k)}_i of the stretch k lies in.  mutant: one deliberate mistake (MUTANTS; "other_ladder" takes another problem's)."""
    visited, obs_t, n_pts = walk["visited"], walk["obs_t"], walk["n_pts"]
    if mutant == "no_gather":      # the states walked on without the ancestors' gathers
        visited = walk["ungathered"]
    lad = np.asarray(other_ladder if mutant == "other_ladder" else ladder, dtype=float)
    qtab = integer_descendant_weights(quantise(walk["lw"]), walk["ancestors"], walk["resampled"])
    kept = np.arange(0, n_pts, stride)
    cursor = np.arange(kept.size) if mutant == "stride_cursor" else kept
    stretch = np.searchsorted(obs_t, cursor, side="left")      # j(k) = #{observations before k}
    if mutant == "final_weights":
        stretch = np.full(kept.size, obs_t.size)
    bins = bins_of(np.swapaxes(visited[kept], 0, 1), lad, "le" if mutant == "le" else "lt")
    if mutant == "drop_last":
        bins = np.minimum(bins, lad.shape[1] - 1)
    mass = np.zeros((kept.size, visited.shape[2], lad.shape[1] + 1), dtype=np.uint64)
    return add_mass(mass, bins, qtab[stretch].T)


def particle_marginals_numpy(problem, x, x0, n, seed, ess_fraction, ladder, stride=1, index=0):
    """One problem's marginals with counter word `index`: particle_moments_numpy's dict (lw, state, ess, resampled, ancestors, m1, lineage_ess,
    ...) plus paths (n, Np, D): the path each final slot's lineage carried, q (n,) uint64, mass (n_keep, D, L + 1) uint64."""
    out = dict(particle_moments_numpy(problem, x, x0, n, seed, ess_fraction, index=index))
    paths = rewalk_numpy(problem, x, x0, seed, trace_slots(np.arange(n), out["ancestors"], out["resampled"]), index=index)
    w = np.exp(out["lw"] - out["lw"].max())
    w = w / w.sum()
    # the paths the moments restatement carried, to the bit: the same sums of the same products
    assert np.array_equal(np.einsum("i,ikd->kd", w, paths), out["m1"]) and np.array_equal(np.einsum("i,ikd->kd", w, paths * paths), out["m2"])
    assert np.array_equal(paths[:, -1], out["state"])
    ladder = np.asarray(ladder, dtype=float).reshape(int(problem.dim_d), -1)
    q = quantise(out["lw"])
    out.update(paths=paths, q=q, ladder=ladder, mass=mass_of_paths(paths, q, ladder, stride))
    return out


def cdf_of(mass):
    """(n_keep, D, L): the integer prefix sums over the total"""
    cum = np.cumsum(mass, axis=2, dtype=np.uint64)
    return cum[:, :, :-1].astype(float) / cum[:, :, -1:].astype(float)


def ladder_of(visited, n_levels):
    """(D, L): the recipe of the module docstring from visited states (..., D)"""
    flat = visited.reshape(-1, visited.shape[-1])
    at = np.array([0.5]) if n_levels == 1 else np.linspace(0.1, 0.9, n_levels)
    return np.stack([np.quantile(np.unique(flat[:, j]), at) for j in range(flat.shape[1])])


def splitting_level(visited, paths, q):
    """(D, 1): ladder_of(visited, 1); where that leaves the surviving lineages (q > 0) of paths (n, Np, D) in one bin at every grid index and
    component, the level of one component becomes the midpoint of the widest gap, relative to max(1, |x|), between two consecutive sorted
    survivors' states at one grid index: then that index and component hold two non-empty bins"""
    lad = ladder_of(visited, 1)
    alive = paths[q > 0]
    if alive.shape[0] < 2:
        return lad
    bins = bins_of(alive, lad)
    if np.any(bins.max(axis=0) != bins.min(axis=0)):
        return lad
    srt = np.sort(alive, axis=0)
    gaps = np.diff(srt, axis=0) / np.maximum(1.0, np.abs(srt[:-1]))
    i, k, j = np.unravel_index(np.argmax(gaps), gaps.shape)
    assert gaps[i, k, j] > 0.0
    lad[j, 0] = 0.5 * (srt[i, k, j] + srt[i + 1, k, j])
    return lad


# ---- the cases of the GPU tests, each computed once per process (read-only) --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(problem_key):
    """the walk of one GPU case (the keys of test_particle_events_cpu.gpu_cases) with its lineage paths, q and the ladders of LEVEL_COUNTS"""
    q, x, x0, n, seed, frac, index = _built(problem_key)
    walk = walk_numpy(q, x, x0, n, seed, frac, index=index)
    paths = rewalk_numpy(q, x, x0, seed, trace_slots(np.arange(n), walk["ancestors"], walk["resampled"]), index=index)
    qf = quantise(walk["lw"])
    ladders = {c: ladder_of(walk["visited"], c) if c > 1 else splitting_level(walk["visited"], paths, qf) for c in LEVEL_COUNTS}
    walk.update(paths=paths, q=qf, ladders=ladders)
    return walk


def _ungathered(problem_key):
    """visited (Np, n, D) of the walk that never gathers: every slot goes on from its own state"""
    from test_path_weights_cpu import _sigma_diag, _split
    from test_sample_paths_cpu import normals
    q, x, x0, n, seed, frac, index = _built(problem_key)
    d, n_pts, dt = int(q.dim_d), int(q.n_pts), float(q.dt)
    fac = np.linalg.cholesky(_sigma_diag(q) * dt)
    lin_a, off_b = _split(q, x)
    state = reference(problem_key)["visited"][0]
    out = np.empty((n_pts, n, d))
    for k in range(n_pts):
        if k > 0:
            state = (state + dt * (-(state @ lin_a[k - 1].T) + off_b[k - 1])) + normals(seed, k, np.arange(n), index, d) @ fac.T
        out[k] = state
    return out


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SAMPLE, ids=str)
def test_restatement(key):
    q, x, x0, n, seed, frac, index = _built(key)
    ref = reference(key)
    flt = particle_filter_numpy(q, x, x0, n, seed, frac, index=index)
    for stride, count in ((1, 7), (4, 63), (int(q.n_pts) + 3, 1)):
        ladder = ref["ladders"][count]
        got = particle_marginals_numpy(q, x, x0, n, seed, frac, ladder, stride=stride, index=index)
        for name in ("lw", "state", "ess", "resampled", "ancestors"):
            assert np.array_equal(got[name], flt[name]), (key, name)
        assert got["margins"] == flt["margins"] and np.array_equal(got["paths"], ref["paths"]) and np.array_equal(got["q"], ref["q"])
        mass = got["mass"]
        n_keep = (int(q.n_pts) - 1) // stride + 1
        assert mass.dtype == np.uint64 and mass.shape == (n_keep, int(q.dim_d), count + 1)
        # the integer histogram of the n final lineages' paths weighted by q, entry by entry in Python integers
        want = np.zeros(mass.shape, dtype=object)
        bins = bins_of(ref["paths"][:, ::stride], ladder)
        for i in range(n):
            for kp in range(0, n_keep, max(1, n_keep // 5)):
                for j in range(mass.shape[1]):
                    want[kp, j, bins[i, kp, j]] += int(ref["q"][i])
        for kp in range(0, n_keep, max(1, n_keep // 5)):
            assert np.array_equal(mass[kp].astype(object), want[kp]), (key, stride, kp)
        # the backward integer recursion over the restatement's ancestors gives the same mass
        assert np.array_equal(mass_backward(ref, ladder, stride), mass), (key, stride)
        # sum_b mass: the same for every component and for every kept k of a stretch (here: of the window -- every row of Q sums to sum q)
        total = mass.sum(axis=2, dtype=np.uint64)
        assert np.all(total == ref["q"].sum(dtype=np.uint64)), (key, stride)
        # (the normalised weights sum to 1 within n roundings, each truncation loses less than 1: nothing can overflow)
        assert 2 ** 62 - n * 2 ** 9 - n <= int(ref["q"].astype(object).sum()) <= 2 ** 62 + n * 2 ** 9 < 2 ** 64
        cdf = cdf_of(mass)
        assert np.all(np.diff(cdf, axis=2) >= 0.0) and cdf.min() >= 0.0 and cdf.max() <= 1.0


def test_nan_and_the_ends_of_the_ladder():
    lad = np.array([[-1.0, 0.0, 2.0]])
    vals = np.array([[-5.0], [-1.0], [-0.5], [0.0], [2.0], [2.5], [np.nan], [np.inf], [-np.inf]])
    assert np.array_equal(bins_of(vals, lad)[:, 0], [0, 0, 1, 1, 2, 3, 0, 3, 0])
    assert np.array_equal(bins_of(vals, lad, "le")[:, 0], [0, 1, 1, 2, 3, 3, 0, 3, 0])


# ---- 2. the exact anchor: a linear-Gaussian chain --------------------------------------------------------------------------------------------
def test_rts_anchor():
    """the OU fixture of test_particle_moments_cpu.test_rts_anchor (A_t = theta, b_t = 0, 4096 particles, seeds 1 .. 16, grid indices 0, an
    observation, a mid-gap index, Np - 1): the seed-mean of the CDF at mean + {-2, -1, -0.5, 0, 0.5, 1, 2} sd of the exact marginal within 4
    standard errors of Phi"""
    q, _, _ = case("ou_euler")
    n = int(q.n_pts)
    x = np.concatenate((np.full(n, float(q.theta)), np.zeros(n)))
    ms, ps = rts_marginals(q)
    t = np.asarray(q.obs_t, dtype=int).ravel()
    at = np.array([0, t[0], (t[0] + t[1]) // 2, n - 1])
    z = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0])
    cdfs = np.empty((16, at.size, z.size))
    for s in range(1, 17):
        run = None
        for a, k in enumerate(at):
            ladder = (ms[k] + z * np.sqrt(ps[k]))[None, :]
            if run is None:
                run = particle_marginals_numpy(q, x, None, 4096, s, 0.5, ladder)
                mass = run["mass"]
            else:
                mass = mass_of_paths(run["paths"], run["q"], ladder)
            cdfs[s - 1, a] = cdf_of(mass)[k, 0]
    mean, se = cdfs.mean(axis=0), cdfs.std(axis=0, ddof=1) / 4.0
    for a, k in enumerate(at):
        print("grid index", k, " Phi", np.round(ndtr(z), 5), " seed-mean", np.round(mean[a], 5), " standard error", np.round(se[a], 5))
    assert np.all(np.abs(mean - ndtr(z)[None, :]) <= 4.0 * se)


# ---- 3. the mutants ----------------------------------------------------------------------------------------------------------------------
def _on_a_visited_state(ref, ladder):
    """the ladder with one level of one component moved onto a state a surviving lineage visits: strictly increasing still"""
    lad = ladder.copy()
    alive = np.flatnonzero(ref["q"] > 0)
    for j in range(lad.shape[0]):
        for l in range(lad.shape[1]):
            lo = lad[j, l - 1] if l > 0 else -np.inf
            hi = lad[j, l + 1] if l + 1 < lad.shape[1] else np.inf
            vals = ref["paths"][alive][:, :, j].ravel()
            inside = vals[(vals > lo) & (vals < hi)]
            if inside.size:
                lad[j, l] = inside[0]
                return lad
    raise AssertionError("no level can be moved onto a visited state")


@pytest.mark.parametrize("key", SAMPLE, ids=str)
def test_mutants_change_the_mass(key):
    """every deliberate mistake changes mass on every case of the sample: fixtures, quiet, placement and batch cases"""
    ref = dict(reference(key))
    ref["ungathered"] = _ungathered(key)
    ladder = ref["ladders"][7]
    good = mass_backward(ref, ladder, 4)
    assert np.array_equal(good, mass_of_paths(ref["paths"], ref["q"], ladder, 4))
    resampled_early = bool(np.any(ref["resampled"]))
    for mutant in MUTANTS:
        if mutant == "le":      # (decided by a state exactly on a level)
            lad = _on_a_visited_state(ref, ladder)
            assert not np.array_equal(mass_backward(ref, lad, 1, mutant), mass_backward(ref, lad, 1)), (key, mutant)
            continue
        if mutant in ("final_weights", "no_gather") and not resampled_early:
            continue      # (nothing was resampled: there is no gather and every row of Q is q)
        assert not np.array_equal(mass_backward(ref, ladder, 4, mutant), good), (key, mutant, family(key))
    assert resampled_early or family(key) == "placement", key      # (the sample's cases resample, but a placement case with a given start may not)


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_mutant_another_problems_ladder(model, d):
    refs = [reference(("batch", model, d, 20, k)) for k in range(3)]
    for k in range(3):
        mine, other = refs[k]["ladders"][7], refs[(k + 1) % 3]["ladders"][7]
        assert not np.array_equal(mass_backward(refs[k], mine, 4, "other_ladder", other), mass_backward(refs[k], mine, 4)), (model, k)


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "quiet_l96d17"])
def test_a_start_on_a_level_lands_in_that_levels_bin(tag):
    """x0 given = c_l: at grid index 0 every particle lies in bin l (c_l < x is false), in bin l + 1 under `<=`"""
    q, x, x0 = case(tag)
    d = int(q.dim_d)
    x0 = np.reshape(np.asarray(x0, dtype=float), d)
    walk = dict(walk_numpy(q, x, x0, 17, 7, 0.5))
    for l in range(3):
        ladder = x0[:, None] + (np.arange(3) - l)[None, :] * 0.25
        ladder[:, l] = x0
        mass = mass_backward(walk, ladder)
        total = quantise(walk["lw"]).sum(dtype=np.uint64)
        assert np.all(mass[0, :, l] == total) and np.all(mass[0].sum(axis=1, dtype=np.uint64) == total), (tag, l)
        wrong = mass_backward(walk, ladder, 1, "le")
        assert np.all(wrong[0, :, l + 1] == total) and np.all(wrong[0, :, l] == 0), (tag, l)


# ---- the ladders and the conditions on the cases of the GPU tests ----------------------------------------------------------------------------
def test_ladders_and_the_conditions_on_the_cases():
    """for every case the GPU file runs: the ladders are finite and strictly increasing; every case with more than one surviving lineage
    (more than one final slot with q > 0) has, on every ladder -- 1, 7 and 63 levels --, a grid index and a component with at least two
    non-empty bins.  (How often the single level is the median itself and how often splitting_level had to move it is printed.)"""
    moved, cases = 0, 0
    for key in gpu_cases():
        ref = reference(key)
        survivors = int(np.count_nonzero(ref["q"]))
        for count in LEVEL_COUNTS:
            lad = ref["ladders"][count]
            assert lad.shape == (ref["visited"].shape[2], count) and np.all(np.isfinite(lad)) and np.all(np.diff(lad, axis=1) > 0.0), (key, count)
            if survivors > 1:
                filled = np.count_nonzero(mass_of_paths(ref["paths"], ref["q"], lad), axis=2)
                assert filled.max() >= 2, (key, count)
                if count == 1:
                    moved += int(not np.array_equal(lad, ladder_of(ref["visited"], 1)))
                    cases += 1
    print("the single level: the median of the visited values in", cases - moved, "of", cases, "cases with survivors to split, moved between two survivors in", moved)


# ---- 4. the record ------------------------------------------------------------------------------------------------------------------------
def _record(mass, levels, **kw):
    n_keep = mass.shape[0]
    return SmoothingMarginals([-700.0, -701.0], levels, mass, [3, 5], 3, 3 * (n_keep - 1) + 1, [0, 4], [1.5, 1.6, 1.7], [2.0, 1.0], [1, 0], **kw)


def test_record_on_a_hand_made_mass():
    levels = np.array([[-1.0, 0.0, 1.0, 3.0], [0.0, 1.0, 2.0, 3.0]])
    mass = np.array([[[0, 2, 4, 2, 0], [1, 1, 2, 3, 1]],
                     [[8, 0, 0, 0, 0], [0, 0, 0, 0, 8]]], dtype=np.uint64)
    rec = _record(mass, levels)
    assert len(rec) == 2 and np.array_equal(rec.grid, [0, 3]) and rec.mass.dtype == np.uint64 and rec.q_final.dtype == np.uint64
    assert np.array_equal(rec.total(), [[8, 8], [8, 8]]) and rec.total().dtype == np.uint64
    assert np.array_equal(rec.hist(), mass / 8.0) and np.allclose(rec.hist().sum(axis=2), 1.0, rtol=1e-15, atol=0.0)
    cdf = rec.cdf()
    assert cdf.shape == (2, 2, 4) and np.array_equal(cdf[0, 0], [0.0, 0.25, 0.75, 1.0]) and np.array_equal(cdf[0, 1], [0.125, 0.25, 0.5, 0.875])
    assert np.array_equal(rec.exceedance(1), 1.0 - cdf[:, :, 1]) and np.array_equal(rec.exceedance(-1), 1.0 - cdf[:, :, 3])
    # quantile inverts cdf at the levels, and is linear inside the bracketing pair
    for l in range(4):
        for j in range(2):
            if cdf[0, j, l] > (cdf[0, j, l - 1] if l else -1.0):      # (a level whose cdf is reached there first)
                assert rec.quantile(cdf[0, j, l])[0, j] == levels[j, l], (j, l)
    assert rec.quantile(0.5)[0, 0] == 0.5 and rec.quantile(0.125)[0, 0] == -0.5
    # the open end bins: -inf below the first level, +inf above the last
    assert rec.quantile(0.05)[0, 1] == -np.inf and rec.quantile(0.95)[0, 1] == np.inf and rec.quantile(0.0)[0, 0] == levels[0, 0]
    assert np.all(rec.quantile(0.5)[1] == [-np.inf, np.inf])
    lo, hi = rec.band(0.25, 0.75)
    assert lo[0, 0] == 0.0 and hi[0, 0] == 1.0 and np.array_equal(lo, rec.quantile(0.25)) and np.array_equal(hi, rec.quantile(0.75))
    assert np.array_equal(rec.lineage_ess_on_grid(), [1.5, 1.6])
    one = SmoothingMarginals([0.0], levels[:1], mass[:, :1], [8], 3, 4, [], [1.0], single_dim=True)
    assert one.cdf().shape == (2, 4) and one.hist().shape == (2, 5) and one.total().shape == (2,) and one.quantile(0.5).shape == (2,)
    assert one.exceedance(0).shape == (2,) and one.modes(0) == 1
    for bad in (lambda: _record(mass.astype(float), levels), lambda: _record(mass[:, :, :4], levels), lambda: _record(mass, levels[:, ::-1]),
                lambda: SmoothingMarginals([0.0], levels, mass, [3], 2, 5, [], [1.0]), lambda: SmoothingMarginals([0.0, 0.0], levels, mass, [3], 3, 4, [], [1.0]),
                lambda: rec.quantile(1.5), lambda: rec.band(0.9, 0.1), lambda: rec.modes(1), lambda: rec.modes(6)):
        with pytest.raises(ValueError):
            bad()


def test_modes_tell_a_bimodal_mass_from_a_unimodal_one():
    levels = np.array([np.linspace(-2.0, 2.0, 9), np.array([-2.0, -1.5, -1.2, -0.4, 0.0, 0.1, 0.9, 1.5, 2.0])])
    uni = [0, 1, 3, 6, 9, 9, 6, 3, 1, 0]           # a plateau at the top: one mode
    bi = [1, 2, 8, 3, 1, 1, 4, 9, 2, 5]            # two humps (the open end bins have no density)
    mass = np.array([[uni, uni], [bi, bi], [[0, 0, 0, 0, 7, 0, 0, 0, 0, 0]] * 2, [[7] + [0] * 9] * 2], dtype=np.uint64)
    rec = SmoothingMarginals([0.0], levels, mass, [9], 1, 4, [], [1.0])
    assert rec.modes(0)[0] == 1 and np.array_equal(rec.modes(2), [1, 1]) and np.array_equal(rec.modes(3), [0, 0])
    assert rec.modes(1)[0] == 2
    # on the uneven ladder the density is mass / width: 8 / 0.3, 3 / 0.8, 1 / 0.4, 1 / 0.1, 4 / 0.8, 9 / 0.6, 2 / 0.5 -> maxima at 8 / 0.3, 1 / 0.1, 9 / 0.6
    assert rec.modes(1)[1] == 3


def test_gaussian_ladder():
    rng = np.random.default_rng(3)
    mt, var = rng.standard_normal((50, 3)), rng.uniform(0.1, 2.0, (50, 3))
    st = np.zeros((50, 3, 3))
    st[:, np.arange(3), np.arange(3)] = var
    for count, width in ((31, 4.0), (2, 1.64), (63, 6.0)):
        lad = gaussian_ladder(mt, st, count, width)
        assert lad.shape == (3, count) and np.all(np.diff(lad, axis=1) > 0.0)
        assert np.all(lad[:, 0] <= np.min(mt - width * np.sqrt(var), axis=0)) and np.all(lad[:, -1] >= np.max(mt + width * np.sqrt(var), axis=0))
        assert np.array_equal(lad, gaussian_ladder(mt, var, count, width))
        assert np.allclose(np.diff(lad, axis=1), (lad[:, -1:] - lad[:, :1]) / (count - 1), rtol=1e-9)
    assert gaussian_ladder(mt[:, 0], var[:, 0]).shape == (1, 31) and gaussian_ladder(mt, st, 1).shape == (3, 1)
    for bad in (lambda: gaussian_ladder(mt, var[:, :2]), lambda: gaussian_ladder(mt, st, 0), lambda: gaussian_ladder(mt, st, 5, 0.0)):
        with pytest.raises(ValueError):
            bad()


# ---- 5. the surface --------------------------------------------------------------------------------------------------------------------------
PROTOTYPE = ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed, "
             "double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, const double* levels, int32_t n_levels, "
             "double* logw, double* state, uint64_t* mass, uint64_t* qfinal_or_null, double* lineage_ess_or_null, double* ess_or_null, "
             "int32_t* resampled_or_null")


def test_symbol_and_prototype():
    assert "vgpa_particle_marginals" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_marginals\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    assert " ".join(proto.group(1).split()) == PROTOTYPE
    assert callable(va.load().vgpa_particle_marginals)


class _Recorder:
    """test_particle_api_cpu.Recorder for this entry: its ladders are (B, D, L), read while they are alive"""

    def __init__(self, n_levels):
        self.calls, self.sizes = [], {"x": B * LEN_X, "x0": B * D, "prior_mu": B * D, "prior_tau": B * D * D, "levels": B * D * n_levels}

    def __getattr__(self, entry):
        def call(*args):
            seen = {}
            for (name, _), arg in zip(prototype(entry), args):
                if name in self.sizes and arg is not None:
                    seen[name] = np.frombuffer(ctypes.string_at(arg.value, self.sizes[name] * 8), dtype=np.float64).copy()
            self.calls.append((entry, args, seen))
            return 0
        return call


def _fake_context(n_levels):
    c = object.__new__(va.Context)
    c._lib, c._h = _Recorder(n_levels), HANDLE
    c.B, c.D, c.Np, c.n_obs, c.len_x = B, D, NP, M, LEN_X
    return c


LADDERS = {"(L,)": np.array([-1.0, 0.0, 0.5, 2.0]), "(D, L)": np.cumsum(np.random.default_rng(5).uniform(0.1, 1.0, (D, 5)), axis=1),
           "(B, D, L)": np.cumsum(np.random.default_rng(6).uniform(0.1, 1.0, (B, D, 63)), axis=2), "(B, D, 1)": np.arange(B * D, dtype=float).reshape(B, D, 1)}


@pytest.mark.parametrize("shape", list(LADDERS))
def test_call_layout(shape):
    """Context.particle_marginals against the header's prototype, position by position (the checks of test_particle_api_cpu.test_call_layout)"""
    levels = LADDERS[shape]
    count = levels.shape[-1]
    ctx = _fake_context(count)
    res = ctx.particle_marginals(N, API_SEED, levels, stride=STRIDE, ess_fraction=ESS_FRACTION, x=X, x0=X0, prior=PRIOR)
    assert [entry for entry, _, _ in ctx._lib.calls] == ["vgpa_particle_marginals"]
    _, args, seen = ctx._lib.calls[0]
    params, argtypes = prototype("vgpa_particle_marginals"), va.load().vgpa_particle_marginals.argtypes
    assert len(args) == len(argtypes) == len(params) == 18 and args[0] is HANDLE
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
            assert argtype is ctypes.c_int32 and type(arg) is int and -2 ** 31 <= arg < 2 ** 31, name
    scalars = {"n_paths": N, "stride": STRIDE, "seed": API_SEED, "ess_fraction": ESS_FRACTION, "n_levels": count}
    assert {name for name, kind in params if kind != "ptr"} == set(scalars)
    for name, value in scalars.items():
        assert at[name] == value, name
    wide = np.broadcast_to(levels if levels.ndim > 1 else levels[None, :], (B, D, count))
    ins = {"x": X, "x0": X0, "prior_mu": PRIOR[0], "prior_tau": PRIOR[1], "levels": wide}
    assert set(seen) == set(ins)
    for name, value in ins.items():
        assert np.array_equal(seen[name], np.asarray(value).ravel()), name
    outs = {"logw": ("log_w", (B, N), np.float64, None), "state": ("state", (B, N, D), np.float64, None), "ess": ("ess", (B, M), np.float64, 0),
            "resampled": ("resampled", (B, M), np.int32, 0), "mass": ("mass", (B, N_KEEP, D, count + 1), np.uint64, None),
            "qfinal": ("q_final", (B, N), np.uint64, None), "lineage_ess": ("lineage_ess", (B, M + 1), np.float64, 0)}
    for name, (key, shp, dtype, fill) in outs.items():
        arr = res[key]
        assert at[name] is not None and at[name].value == arr.ctypes.data, name
        assert arr.shape == shp and arr.dtype == dtype and arr.flags["C_CONTIGUOUS"], name
        assert fill is None or np.all(arr == fill), name
    assert {name for name, kind in params if kind == "ptr"} - {"ctx"} == set(ins) | set(outs)
    assert list(res) == ["log_w", "state", "ess", "resampled", "mass", "q_final", "lineage_ess"]
    bare = _fake_context(count)
    bare.particle_marginals(N, API_SEED, levels)
    names = [name for name, _ in params]
    for name in ("x", "x0", "prior_mu", "prior_tau"):
        assert bare._lib.calls[0][1][names.index(name)] is None, name
    assert bare._lib.calls[0][1][names.index("stride")] == 1 and bare._lib.calls[0][1][names.index("ess_fraction")] == 0.5


def test_refusals_by_text_and_order():
    """what Context.particle_marginals refuses before it reaches the library: the integers first, then the ladder, then x"""
    ctx = _fake_context(4)
    good, bad_x = LADDERS["(L,)"], np.zeros((B, LEN_X + 1))
    refusals = [
        (dict(n_paths=2 ** 31, levels=np.zeros((2, 2, 2, 2)), x=bad_x), "n_paths and stride must fit into 32 bits"),
        (dict(levels=np.zeros((2, 2, 2, 2)), x=bad_x), r"levels has shape \(2, 2, 2, 2\), expected \(L,\), \(3, L\) or \(2, 3, L\)"),
        (dict(levels=np.zeros(0), x=bad_x), r"levels has shape \(0,\), expected"),
        (dict(levels=np.zeros((4, 5)), x=bad_x), r"levels has shape \(4, 5\), expected \(5,\), \(3, 5\) or \(2, 3, 5\)"),
        (dict(levels=np.arange(64.0), x=bad_x), "levels holds 64 levels per component, expected 1 to 63"),
        (dict(levels=np.array([0.0, np.inf]), x=bad_x), "levels must be finite"),
        (dict(levels=np.array([0.0, np.nan, 1.0]), x=bad_x), "levels must be finite"),
        (dict(levels=np.array([0.0, 1.0, 1.0]), x=bad_x), r"levels must be strictly increasing \(problem 0, component 0\)"),
        (dict(levels=np.stack([np.tile([0.0, 1.0], (3, 1)), np.array([[0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])]), x=bad_x),
         r"levels must be strictly increasing \(problem 1, component 2\)"),
        (dict(levels=good, x=bad_x), "x has 266 entries, expected 264"),
    ]
    for kw, text in refusals:
        args = dict(n_paths=N, seed=1, levels=good)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            ctx.particle_marginals(args.pop("n_paths"), args.pop("seed"), args.pop("levels"), **args)
    assert ctx._lib.calls == []
    assert _lib.MAX_MARGINAL_LEVELS == 63


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "levels", "stride", "ess_fraction", "x", "x0", "prior"]),
                          (va.VarGP, ["n_paths", "seed", "levels", "stride", "ess_fraction", "x", "x0", "n_levels", "width"]),
                          (va.ProblemBatch, ["n_paths", "seed", "levels", "stride", "ess_fraction", "x", "x0", "n_levels", "width"])]:
        fn = getattr(owner, "particle_marginals", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["stride"].default == 1
        if owner is not va.Context:
            assert sig["levels"].default is None and sig["n_levels"].default == 31 and sig["width"].default == 4.0
    assert va.SmoothingMarginals is SmoothingMarginals and "SmoothingMarginals" in va.__all__
    sig = inspect.signature(gaussian_ladder).parameters
    assert list(sig) == ["mt", "st", "n_levels", "width"] and sig["n_levels"].default == 31 and sig["width"].default == 4.0
    for name in ("total", "cdf", "hist", "exceedance", "quantile", "band", "modes", "lineage_ess_on_grid", "log_evidence"):
        assert callable(getattr(SmoothingMarginals, name)), name
    from vgpa_amd.particles import _GenealogySums, _KeptGrid, _WalkRecord
    assert issubclass(SmoothingMarginals, _GenealogySums) and issubclass(SmoothingMarginals, _KeptGrid) and issubclass(SmoothingMarginals, _WalkRecord)
