"""
Whole smoothing trajectories from the particle filter's genealogy (vgpa_particle_paths): the numpy restatements, their checks against the
filter and the moments they ride on, the pick of the final slots, the margin condition of the GPU tests, an exact anchor on a linear chain,
the record SmoothingPaths and the host-side surface.

Two restatements, which the device must both agree with:
  particle_paths_numpy   the forward algorithm -- the walk of particle_ref.FilterWalk, in which every slot carries its whole path and,
                         beside it, the slot its lineage sat in during every stretch; a resampling copies both through the same `anc`
                         as the states.  What the trajectories ARE.
  trace_slots + rewalk_numpy   what the device does: the final slots traced backwards through the stored ancestors, then every trajectory
                         walked alone from the counters of its slots, nothing carried and nothing gathered.
test_trace_and_rewalk_is_the_forward_algorithm asserts that the two give the same bits, so the GPU tests may use the second (which costs K
paths, not n) on the histories of the first.

pick_slots: the K final slots by systematic resampling from the final weights, as vgpa_hip.h states it.  The device forms the prefix sums
in another association than np.cumsum, so its slots are the restatement's where every threshold keeps a margin from every prefix sum:
test_margin_condition asserts >= 1e-7 S, the bound of the filter's own tests, for every run of tests/test_particle_paths.py in drawn mode.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import SmoothingPaths
from conftest import ROOT
from particle_ref import FilterWalk
from test_particle_filter_cpu import FRACTIONS, MARGIN, QUIET, SEED, case, particle_filter_numpy
from test_particle_filter_cpu import reference as filter_reference
from test_particle_moments_cpu import particle_moments_numpy, rts_marginals
from test_path_weights_cpu import TAGS, _sigma_diag, _split, obs_model
from test_sample_paths_cpu import em_noise, em_step, philox4x32_10, start_cloud, unit_open

CASES = [(t, s) for t in TAGS for s in ("given", "drawn")] + [(t, "given") for t in QUIET]
# (particles, trajectories) of the GPU tests in drawn mode: one particle; more trajectories than particles and a second workgroup above
# D = 4; a partial wave; one trajectory; a partial 64-path block behind a full one
DRAWN = [(1, 17), (17, 65), (65, 17), (300, 1), (300, 65)]


def particle_paths_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`, every slot carrying its path and its lineage's slots.  Returns FilterWalk.record's
    dict with paths (n, Np, D): the path of the lineage that ends in each final slot, and table (M + 1, n): the slot that lineage sat in
    during every stretch (row M: the final slot)."""
    walk = FilterWalk(problem, x, x0, n, seed, ess_fraction, index)
    paths = np.zeros((n, walk.n_pts, walk.d))
    table = np.full((walk.obs_t.size + 1, n), -1, dtype=np.int64)
    for event, i in walk:
        if event in ("start", "step"):
            paths[:, i] = walk.state
        elif event == "cut":
            table[i] = np.arange(n)         # stretch i ends here: the slot the lineage is in
        elif event == "gather":
            paths, table = paths[walk.anc], table[:, walk.anc]
    table[-1] = np.arange(n)
    return walk.record(paths=paths, table=table)


def trace_slots(final, ancestors, resampled):
    """(M + 1, K): row M = final; row j = ancestors[j][row j + 1] where resampled[j], else row j + 1 (step 2 of vgpa_hip.h)"""
    final = np.asarray(final, dtype=np.int64).ravel()
    flags = np.asarray(resampled).astype(bool).ravel()
    anc = np.asarray(ancestors, dtype=np.int64).reshape(flags.size, -1)
    out = np.empty((flags.size + 1, final.size), dtype=np.int64)
    out[-1] = final
    for j in range(flags.size - 1, -1, -1):
        out[j] = anc[j][out[j + 1]] if flags[j] else out[j + 1]
    return out


def rewalk_numpy(problem, x, x0, seed, table, index=0):
    """(K, Np, D): every trajectory walked alone (step 3 of vgpa_hip.h): the start with the counter word table[0], the step to k with
    table[j(k)], j(k) = #{observations before k}.  The unweighted recursion of sample_paths_numpy, its operations in the filter's order."""
    n_pts, dt = int(problem.n_pts), float(problem.dt)
    fac = np.linalg.cholesky(_sigma_diag(problem) * dt)
    lin_a, off_b = _split(problem, x)
    obs_t = np.asarray(obs_model(problem)[0], dtype=np.int64)
    table = np.asarray(table, dtype=np.int64)
    assert table.shape[0] == obs_t.size + 1
    state = start_cloud(problem, x0, seed, table[0], index)
    out = np.empty((table.shape[1], n_pts, int(problem.dim_d)))
    out[:, 0] = state
    for k in range(1, n_pts):
        j = int(np.searchsorted(obs_t, k, side="left"))
        state = em_step(state, dt, -(state @ lin_a[k - 1].T) + off_b[k - 1], em_noise(seed, k, table[j], index, fac))
        out[:, k] = state
    return out


def pick_slots(lw, n_draw, seed, n_pts, index=0, u01=None):
    """(slots (K,), margin): step 1 of vgpa_hip.h, the count written out; margin = min_{m,i} |u_m - cum_i| / S"""
    lw = np.asarray(lw, dtype=float).ravel()
    n = lw.size
    w = np.exp(lw - lw.max())
    cum = np.cumsum(w)
    total = cum[-1]
    if u01 is None:
        rr = philox4x32_10((n_pts, 0, index, 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        u01 = float(unit_open(rr[0], rr[1]))
    u = (u01 + np.arange(n_draw)) / n_draw * total
    count = np.sum(cum[None, :] <= u[:, None], axis=1)
    margin = float(np.min(np.abs(u[:, None] - cum[None, :])) / total)
    return np.minimum(count, n - 1), margin


def scale_of(paths):
    """(K, 1, 1): the largest |x| of each trajectory -- what its rounding errors are proportional to"""
    return np.max(np.abs(paths), axis=(1, 2), keepdims=True)


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """the forward restatement of a case of test_particle_filter_cpu.case, computed once per process (read-only)"""
    q, x, x0 = case(tag)
    return particle_paths_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "quiet_l96d12"])
def test_same_walk_as_the_filter_and_the_moments(tag):
    q, x, x0 = case(tag)
    for start in (None, x0):
        for frac in (0.0, 0.5, 1.0):
            got = particle_paths_numpy(q, x, start, 17, SEED, frac)
            want = particle_filter_numpy(q, x, start, 17, SEED, frac)
            for key in ("lw", "state", "ess", "resampled", "ancestors"):
                assert np.array_equal(got[key], want[key]), (tag, frac, key)
            assert np.array_equal(got["clouds"], want["clouds"]) and got["margins"] == want["margins"]
            mom = particle_moments_numpy(q, x, start, 17, SEED, frac)
            w = np.exp(got["lw"] - got["lw"].max())
            w = w / w.sum()
            assert np.array_equal(np.einsum("i,ikd->kd", w, got["paths"]), mom["m1"]), (tag, frac)
            assert np.array_equal(np.einsum("i,ikd->kd", w, got["paths"] * got["paths"]), mom["m2"]), (tag, frac)
            # the contract of vgpa_hip.h, on the restatement itself
            for j, t in enumerate(got["obs_t"]):
                assert np.array_equal(got["paths"][:, t], got["clouds"][j][got["table"][j]]), (tag, frac, j)
            assert np.array_equal(got["paths"][:, -1], got["state"]) and np.array_equal(got["table"][-1], np.arange(17))


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("ess_fraction", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "quiet_l96d12"])
def test_trace_and_rewalk_is_the_forward_algorithm(tag, ess_fraction, start):
    """the table traced backwards through the histories is the carried one, and a lane that walks alone with its slots' counters arrives,
    bit for bit, at the path the forward algorithm carried into every final slot"""
    q, x, x0 = case(tag)
    s0 = x0 if start == "given" else None
    for n in (17, 65):
        fwd = particle_paths_numpy(q, x, s0, n, SEED, ess_fraction)
        table = trace_slots(np.arange(n), fwd["ancestors"], fwd["resampled"])
        assert np.array_equal(table, fwd["table"]), (tag, n)
        assert np.array_equal(rewalk_numpy(q, x, s0, SEED, table), fwd["paths"]), (tag, n)
        if ess_fraction > 0.0 and tag not in QUIET:
            assert fwd["resampled"].any() and np.unique(table[0]).size < n      # (the genealogy has coalesced: the table is no identity)


# ---- the pick ------------------------------------------------------------------------------------------------------------------------------
def test_pick_on_a_hand_made_table():
    lw = np.log([1.0, 2.0, 3.0, 4.0]) - 700.0      # w = 1/4, 1/2, 3/4, 1: cum = 1/4, 3/4, 3/2, 5/2
    slots, margin = pick_slots(lw, 5, 0, 0, u01=0.3)   # u = 0.15, 0.65, 1.15, 1.65, 2.15
    assert np.array_equal(slots, [0, 1, 2, 3, 3]) and abs(margin - 0.1 / 2.5) <= 1e-12
    assert np.array_equal(pick_slots(lw, 1, 0, 0, u01=0.05)[0], [0]) and np.array_equal(pick_slots(lw, 1, 0, 0, u01=0.95)[0], [3])
    assert np.array_equal(pick_slots(lw, 2, 0, 0, u01=1.0)[0], [2, 3])      # (u = S: four sums <= u, the slot is clipped to n - 1)
    assert np.array_equal(pick_slots([-3.0], 4, 0, 0, u01=0.5)[0], [0, 0, 0, 0])
    # more trajectories than particles: each slot about K w_i / S times
    slots, _ = pick_slots(lw, 40, 0, 0, u01=0.5)
    assert np.array_equal(np.bincount(slots, minlength=4), [4, 8, 12, 16]) and np.all(np.diff(slots) >= 0)
    # the uniform is the first one of counter (Np, 0, p, 0xffffffff)
    rr = philox4x32_10((101, 0, 2, 0xFFFFFFFF), (SEED, 0))
    assert np.array_equal(pick_slots(lw, 7, SEED, 101, index=2)[0], pick_slots(lw, 7, 0, 0, u01=float(unit_open(rr[0], rr[1])))[0])


@pytest.mark.parametrize("tag", ["ou_euler", "l96d12_euler_p", "quiet_l96d12"])
def test_pick_against_searchsorted(tag):
    q = case(tag)[0]
    for n, k in DRAWN:
        lw = filter_reference(tag, "given", n, 0.5)["lw"]
        slots, _ = pick_slots(lw, k, SEED, int(q.n_pts))
        w = np.exp(lw - lw.max())
        rr = philox4x32_10((int(q.n_pts), 0, 0, 0xFFFFFFFF), (SEED, 0))
        u = (float(unit_open(rr[0], rr[1])) + np.arange(k)) / k * np.cumsum(w)[-1]
        assert np.array_equal(slots, np.minimum(np.searchsorted(np.cumsum(w), u, side="right"), n - 1)), (tag, n, k)
        assert np.all(np.diff(slots) >= 0) and slots.min() >= 0 and slots.max() < n


def drawn_runs():
    """every (case, start, particles, trajectories, ess_fraction) tests/test_particle_paths.py runs in drawn mode; the seed is SEED"""
    return [(tag, start, n, k, frac) for tag, start in CASES for n, k in DRAWN for frac in FRACTIONS]


def test_margin_condition():
    """a condition on the cases, not a measurement of the device: every threshold of the pick keeps at least 1e-7 S from every prefix sum
    (the filter's own resamplings in these runs: the (case, n, seed) with n in SIZES are cleared by
    test_particle_filter_cpu.test_margin_condition; n = 1 resamples nothing)"""
    smallest = np.inf
    for tag, start, n, k, frac in drawn_runs():
        ref = filter_reference(tag, start, n, frac)
        assert not ref["margins"] or min(ref["margins"]) >= MARGIN, (tag, start, n, frac)
        margin = pick_slots(ref["lw"], k, SEED, int(case(tag)[0].n_pts))[1]
        smallest = min(smallest, margin)
        assert margin >= MARGIN, (tag, start, n, k, frac, margin)
    print("smallest margin of the picks:", smallest, "over", len(drawn_runs()), "runs")


def test_margin_condition_of_the_other_runs():
    """the drawn picks tests/test_particle_paths.py makes beside drawn_runs(): the placement cases (17 particles, 65 trajectories,
    ess_fraction 1), the batches of three (40 particles, 17 trajectories, SEED_BATCH) and the ProblemBatch members (17 particles, 6
    trajectories, SEED_BATCH).  Their filters' own margins are cleared by test_particle_filter_cpu and test_particle_moments_cpu."""
    from helpers import build_problem
    from test_particle_filter_cpu import PLACEMENTS, SEED_BATCH, batch_case, placement_case
    from test_path_weights import _fields
    smallest = np.inf
    for model, d in (("L63", 3), ("L96", 12)):
        for obs_at in PLACEMENTS:
            q, x = placement_case(model, d, obs_at)
            for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
                lw = particle_filter_numpy(q, x, x0, 17, SEED, 1.0)["lw"]
                smallest = min(smallest, pick_slots(lw, 65, SEED, int(q.n_pts))[1])
        for first in (20, 50):
            probs, xs = batch_case(model, d, first)
            for k in range(3):
                lw = particle_filter_numpy(probs[k], xs[k], None, 40, SEED_BATCH, 0.5, index=k)["lw"]
                smallest = min(smallest, pick_slots(lw, 17, SEED_BATCH, int(probs[k].n_pts), index=k)[1])
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    for k, p in enumerate(ps):
        q = _fields(p["vgp"])
        lw = particle_filter_numpy(q, p["vgp"].initialization(), None, 17, SEED_BATCH, 0.5, index=k)["lw"]
        smallest = min(smallest, pick_slots(lw, 6, SEED_BATCH, int(q.n_pts), index=k)[1])
    print("smallest margin of the other picks:", smallest)
    assert smallest >= MARGIN


# ---- the exact anchor: a linear-Gaussian chain ---------------------------------------------------------------------------------------------
def test_rts_anchor():
    """4096 particles, 4096 drawn trajectories, 16 seeds: the seed-mean of the mean and of the variance over the drawn trajectories within
    4 standard errors of the exact smoothing marginals at grid indices 0, 33, 50 and 100.  Only the four indices are needed, so the
    trajectories are read off the forward algorithm's histories: index 0 and the observation indices from the clouds, by the table."""
    q, _, _ = case("ou_euler")
    n_pts = int(q.n_pts)
    assert n_pts == 101
    x = np.concatenate((np.full(n_pts, float(q.theta)), np.zeros(n_pts)))      # A_t = theta, b_t = 0: the proposal is the model
    ms, ps = rts_marginals(q)
    at = np.array([0, 33, 50, 100])
    mean, var = [], []
    for seed in range(1, 17):
        fwd = particle_paths_numpy(q, x, None, 4096, seed, 0.5)
        final, _ = pick_slots(fwd["lw"], 4096, seed, n_pts)
        draws = fwd["paths"][final][:, at, 0]          # (the forward algorithm carried every final slot's path)
        mean.append(draws.mean(axis=0))
        var.append(draws.var(axis=0))
    mean, var = np.array(mean), np.array(var)
    se_m, se_v = mean.std(axis=0, ddof=1) / 4.0, var.std(axis=0, ddof=1) / 4.0
    print("exact mean", ms[at], " seed-mean", mean.mean(axis=0), " standard error", se_m)
    print("exact var ", ps[at], " seed-mean", var.mean(axis=0), " standard error", se_v)
    assert np.all(np.abs(mean.mean(axis=0) - ms[at]) <= 4.0 * se_m)
    assert np.all(np.abs(var.mean(axis=0) - ps[at]) <= 4.0 * se_v)


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    paths = np.arange(3 * 4 * 2, dtype=float).reshape(3, 4, 2) ** 1.5
    slots = np.array([[0, 0, 0], [0, 0, 2], [1, 0, 2], [1, 3, 2]])
    rec = SmoothingPaths([-700.0, -701.0, -702.0, -700.5], paths, slots, 3, 11, [0, 4, 10], [2.0, 1.0, 1.5], [1, 0, 0])
    assert len(rec) == 3 and np.array_equal(rec.grid, [0, 3, 6, 9]) and rec.resampled.dtype == bool and rec.drawn
    assert np.array_equal(rec.paths, paths) and np.array_equal(rec.slots, slots)
    assert np.allclose(rec.mean(), paths.mean(axis=0), rtol=1e-14) and np.allclose(rec.var(), paths.var(axis=0), rtol=1e-13)
    w = np.array([1.0, 2.0, 5.0])
    assert np.allclose(rec.mean(w), np.einsum("i,ikd->kd", w / 8.0, paths), rtol=1e-14)
    assert np.allclose(rec.var(w), np.einsum("i,ikd->kd", w / 8.0, (paths - rec.mean(w)) ** 2), rtol=1e-13)
    assert np.array_equal(rec.distinct(), [1, 2, 3, 3])
    # index 0 lies in stretch 0 (k <= t_0 = 0), 3 in stretch 1 (0 < k <= 4), 6 and 9 in stretch 2 (4 < k <= 10)
    assert np.array_equal(rec.distinct_on_grid(), [1, 2, 3, 3])
    fw = np.exp(np.array([-1.0, -0.5, -2.0]))
    assert np.allclose(rec.final_weights(), fw / fw.sum(), rtol=1e-13)
    top = np.log(np.sum(np.exp(np.array([0.0, -1.0, -2.0, -0.5])))) - 700.0 - np.log(4.0)
    assert np.isclose(rec.log_evidence(), top, rtol=1e-14)
    given = SmoothingPaths([-700.0, -701.0, -702.0, -700.5], paths, slots, 3, 11, [0, 4, 10], drawn=False)
    with pytest.raises(ValueError, match="weights"):
        given.mean()
    assert np.allclose(given.mean(given.final_weights()), np.einsum("i,ikd->kd", fw / fw.sum(), paths), rtol=1e-14)
    one = SmoothingPaths([0.0], paths[:, :, :1], np.zeros((1, 3), dtype=int), 3, 11, [], single_dim=True)
    assert one.paths.shape == (3, 4) and one.mean().shape == one.var().shape == (4,) and np.array_equal(one.distinct_on_grid(), np.ones(4))
    for bad in (lambda: SmoothingPaths([], paths, slots, 3, 11, [0, 4, 10]), lambda: SmoothingPaths([0.0] * 4, paths, slots, 2, 11, [0, 4, 10]),
                lambda: SmoothingPaths([0.0] * 4, paths, slots, 0, 11, [0, 4, 10]), lambda: SmoothingPaths([0.0] * 4, paths, slots, 3, 11, [0, 4]),
                lambda: SmoothingPaths([0.0] * 3, paths, slots, 3, 11, [0, 4, 10]), lambda: SmoothingPaths([0.0] * 4, paths, -slots, 3, 11, [0, 4, 10]),
                lambda: SmoothingPaths([0.0] * 4, paths, slots, 3, 11, [0, 4, 10], [1.0], []), lambda: rec.mean([1.0, 2.0]),
                lambda: rec.var([1.0, -2.0, 3.0])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_paths" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_paths\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t n_draw, "
                    "const int32_t* final_slots_or_null, int32_t stride, uint64_t seed, double ess_fraction, const double* prior_mu_or_null, "
                    "const double* prior_tau_or_null, double* logw, double* state, double* paths, int32_t* slots_or_null, double* ess_or_null, "
                    "int32_t* resampled_or_null")


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "n_draw", "stride", "ess_fraction", "x", "x0", "prior", "slots"]),
                          (va.VarGP, ["n_paths", "seed", "n_draw", "stride", "ess_fraction", "x", "x0", "slots"]),
                          (va.ProblemBatch, ["n_paths", "seed", "n_draw", "stride", "ess_fraction", "x", "x0", "slots"])]:
        fn = getattr(owner, "particle_paths", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["ess_fraction"].default == 0.5 and sig["stride"].default == 1 and sig["slots"].default is None
    assert va.SmoothingPaths is SmoothingPaths and "SmoothingPaths" in va.__all__
    assert isinstance(SmoothingPaths.grid, property)
    for name in ("mean", "var", "distinct", "distinct_on_grid", "final_weights", "log_evidence"):
        assert callable(getattr(SmoothingPaths, name))
    assert "collaps" in SmoothingPaths.__doc__      # (the caveat is stated where the user reads it)
