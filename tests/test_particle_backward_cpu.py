"""
Backward-simulation smoothing trajectories (vgpa_particle_backward_paths; forward filtering, backward simulation at the resampled
observations): the numpy restatement, its bit equalities, the gap condition of the GPU tests, an exact anchor on a linear chain, and the
host-side surface.

history_numpy          the walk of particle_ref.FilterWalk with hlw (M, n): every slot's log-weight at the problem's observation j, that
                       observation's term included, before the resampling decision.
backward_slots_numpy   the table as vgpa_hip.h states it: row c the final slots; row j = row j + 1 where the cloud was carried on, else the
                       Gumbel-max draw among all n slots.  Returns, per draw, the gap between the two largest scores b + g.
rewalk_backward_numpy  the trajectories: rewalk_numpy with the reload of the state at every completed observation.

The device forms x~, exp / log and the quadratic form in another order than numpy (about 1e-12 in the scores), so its table is the
restatement's where every draw's winner keeps a gap from the runner-up: test_gap_condition asserts >= 1e-8 (log units) for every run of
tests/test_particle_backward.py -- a condition on the cases, not a measurement of the device.
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
from vgpa_amd.particles import SmoothingPaths
from conftest import ROOT
from particle_ref import FilterWalk
from test_gpu_edge_cases import make_problem
from test_particle_filter_cpu import FRACTIONS, MARGIN, PLACEMENTS, SEED, SEED_BATCH, batch_case, case, placement_case
from test_particle_moments_cpu import rts_marginals
from test_particle_paths_cpu import DRAWN, particle_paths_numpy, pick_slots, rewalk_numpy, trace_slots
from test_path_weights_cpu import FIXTURES, _sigma_diag, _split
from test_sample_paths_cpu import em_noise, em_step, model_drift, normals, philox4x32_10, start_cloud, unit_open

GAP = 1e-8
# the cases of the GPU tests: D = 1, 1, 3, 12, 17, 40 with a drawn start; D = 64 (NT = 64 without a padding row), a quiet case (resampled and
# carried clouds mixed) and Lorenz-63 once more with a given start (every particle of the first cloud's history starts from one state)
BCASES = [(t, "drawn") for t in FIXTURES] + [("l96d64", "given"), ("quiet_l96d12", "given"), ("l63_euler_p", "given")]
# Lorenz-96 where the draw has something to decide (tight_case): D = 12, 40 (above D = 31 the draw's LDS tile admits one workgroup per
# compute unit) and 50 (the matrix-core walk's NT = 64 with 14 padding rows), (particles, trajectories) of DRAWN's three non-trivial pairs
TIGHT = (12, 40, 50)
TIGHT_RUNS = [(17, 65), (65, 17), (300, 65)]
BIG = ("ou_euler", 4096, 4096, 0.5, 436)      # the one large run: the seed of test_particle_filter_cpu.OU_BIG, whose margins that file clears


def history_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """One problem's filter with counter word `index`.  Returns FilterWalk.record's dict with hlw (M, n)."""
    walk = FilterWalk(problem, x, x0, n, seed, ess_fraction, index)
    hlw = np.full((walk.obs_t.size, n), np.nan)
    for event, j in walk:
        if event == "cut":
            hlw[j] = walk.lw
    return walk.record(hlw=hlw)


def gumbels(seed, k, m, index, n):
    """(len(m), n): g_i = -log(-log u_i) of trajectory m at grid index k; u of the slots 2q and 2q + 1 from the one Philox call with counter
    (k, m, index, 0x80000000 | q): unit_open(r0, r1) for the even slot, unit_open(r2, r3) for the odd one"""
    m = np.asarray(m, dtype=np.uint64).ravel()
    pairs = np.arange((n + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((np.uint64(k), m[:, None], np.uint64(index), np.uint64(0x80000000) | pairs[None, :]), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = np.stack((unit_open(r[0], r[1]), unit_open(r[2], r[3])), axis=-1).reshape(m.size, -1)[:, :n]
    return -np.log(-np.log(u))


def argmax_with_gap(score):
    """(the smallest index that attains the row's maximum (K,), the maximum minus the second largest entry (K,); inf for one column)"""
    win = np.argmax(score, axis=1)
    if score.shape[1] == 1:
        return win, np.full(score.shape[0], np.inf)
    top2 = np.partition(score, score.shape[1] - 2, axis=1)[:, -2:]
    return win, top2[:, 1] - top2[:, 0]


def backward_slots_numpy(problem, x, seed, hist, final, index=0, drift=model_drift, divisor=None, target=None):
    """(table (M + 1, K), gaps: one array (K,) per resampled observation).  Row M = final; for j = M-1 .. 0: row j + 1 where the cloud was
    carried on, else per trajectory m the smallest i that attains max_i (b_i + g_i).  drift: the model drift of the transition means
    (another one: how the table reacts to a wrong drift); divisor(rdiag) -> the divisors of the quadratic form and target(z, x~) -> the
    successor the candidates are scored against (z: the trajectory's state at the cut), the hooks of two more mutants."""
    d, dt = int(problem.dim_d), float(problem.dt)
    rdiag = np.linalg.cholesky(_sigma_diag(problem) * dt).diagonal()
    lin_a, off_b = _split(problem, x)
    theta = np.asarray(problem.theta, dtype=float)
    obs_t = hist["obs_t"]
    final = np.asarray(final, dtype=np.int64).ravel()
    n = hist["lw"].size
    table = np.empty((obs_t.size + 1, final.size), dtype=np.int64)
    table[-1] = final
    gaps = []
    for j in range(obs_t.size - 1, -1, -1):
        if not hist["resampled"][j]:
            table[j] = table[j + 1]
            continue
        k, s, cloud = int(obs_t[j]), table[j + 1], hist["clouds"][j]
        z = cloud[hist["ancestors"][j][s]]
        xt = (z + dt * (-(z @ lin_a[k].T) + off_b[k])) + normals(seed, k + 1, s, index, d) * rdiag[None, :]
        if target is not None:
            xt = target(z, xt)
        div = rdiag if divisor is None else divisor(rdiag)
        mu = cloud + dt * drift(problem.model, theta, cloud)
        win, gap = np.empty(final.size, dtype=np.int64), np.empty(final.size)
        for lo in range(0, final.size, 256):      # (256 trajectories at a time: the scores are (256, n))
            hi = min(lo + 256, final.size)
            quad = np.zeros((hi - lo, n))
            for c in range(d):
                quad += ((xt[lo:hi, c, None] - mu[None, :, c]) / div[c]) ** 2
            score = (hist["hlw"][j][None, :] - 0.5 * quad) + gumbels(seed, k, np.arange(lo, hi), index, n)
            win[lo:hi], gap[lo:hi] = argmax_with_gap(score)
        table[j] = win
        gaps.append(gap)
    return table, gaps


def rewalk_backward_numpy(problem, x, x0, seed, table, hist, index=0):
    """(K, Np, D): rewalk_numpy's walk -- the start with the counter word table[0], the step to k with table[j(k)] -- in which the state is
    replaced, behind every completed observation j and after that point is stored, by clouds[j][ancestors[j][table[j + 1]]]"""
    n_pts, dt = int(problem.n_pts), float(problem.dt)
    fac = np.linalg.cholesky(_sigma_diag(problem) * dt)
    lin_a, off_b = _split(problem, x)
    obs_t = hist["obs_t"]
    at = {int(t): j for j, t in enumerate(obs_t)}
    table = np.asarray(table, dtype=np.int64)
    assert table.shape[0] == obs_t.size + 1
    state = start_cloud(problem, x0, seed, table[0], index)
    out = np.empty((table.shape[1], n_pts, int(problem.dim_d)))
    for k in range(n_pts):
        if k > 0:
            j = int(np.searchsorted(obs_t, k, side="left"))
            state = em_step(state, dt, -(state @ lin_a[k - 1].T) + off_b[k - 1], em_noise(seed, k, table[j], index, fac))
        out[:, k] = state
        if k in at:
            state = hist["clouds"][at[k]][hist["ancestors"][at[k]][table[at[k] + 1]]]
    return out


@functools.lru_cache(maxsize=None)
def history(tag, start, n, ess_fraction, seed=SEED):
    """the filter's histories of a case of test_particle_filter_cpu.case, computed once per process (read-only)"""
    q, x, x0 = case(tag)
    return history_numpy(q, x, x0 if start == "given" else None, n, seed, ess_fraction)


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, n_draw, ess_fraction, seed=SEED):
    """(history, final slots, table, smallest gap) of a run with drawn final slots, computed once per process (read-only)"""
    q, x, _ = case(tag)
    hist = history(tag, start, n, ess_fraction, seed)
    final, _ = pick_slots(hist["lw"], n_draw, seed, int(q.n_pts))
    table, gaps = backward_slots_numpy(q, x, seed, hist, final)
    return hist, final, table, min([float(g.min()) for g in gaps], default=np.inf)


@functools.lru_cache(maxsize=None)
def tight_case(d):
    """(problem, x): Lorenz-96 with an observation at grid index 0 whose cloud is tight against the transition density.  In the fixtures
    the particles of a cloud lie many transition widths apart -- their squared distance over R^2 grows with D t_j / dt --, so a successor
    identifies the particle it was copied from and backward simulation returns the genealogy.  Here the start is drawn with
    S0 = 4 Sigma dt / D (the candidates lie about two widths apart in all D components together), the prior is the start's own law and
    the observation noise is wide (the weights are nearly, not exactly, equal: with ess_fraction 1 the cloud is resampled), and dt = 0.05
    makes the drift's share of the transition mean count: the draw at index 0 then depends on x~, on the circular drift and on 1 / R."""
    q, x = make_problem("L96", d, 41, method="euler", dt=0.05, obs_at=[0, 7, 20])
    s0 = np.diag(4.0 * np.asarray(q.sigma, dtype=float).diagonal() * 0.05 / d)
    return dataclasses.replace(q, s0=s0, mu0=np.asarray(q.m0, dtype=float), tau0=s0, obs_noise=100.0 * np.eye(d)), x


@functools.lru_cache(maxsize=None)
def tight_reference(d, n, n_draw):
    """(history, final slots, table, gaps) of a tight case: the start drawn, SEED, ess_fraction 1"""
    q, x = tight_case(d)
    hist = history_numpy(q, x, None, n, SEED, 1.0)
    final, _ = pick_slots(hist["lw"], n_draw, SEED, int(q.n_pts))
    table, gaps = backward_slots_numpy(q, x, SEED, hist, final)
    return hist, final, table, gaps


def backward_runs():
    """every (case, start, particles, trajectories, ess_fraction) tests/test_particle_backward.py runs on the fixtures; the seed is SEED"""
    return [(tag, start, n, k, frac) for tag, start in BCASES for n, k in DRAWN for frac in FRACTIONS]


@functools.lru_cache(maxsize=None)
def other_runs():
    """the draws tests/test_particle_backward.py makes beside backward_runs(), as (label, problem, x, x0, seed, index, history, final):
    the placement cases (17 particles, 65 trajectories, ess_fraction 1), the batches of three (40 particles, 17 trajectories, SEED_BATCH)
    and the ProblemBatch members (17 particles, 6 trajectories, SEED_BATCH)"""
    from helpers import build_problem
    from test_path_weights import _fields
    runs = []
    for model, d in (("L63", 3), ("L96", 12)):
        for obs_at in PLACEMENTS:
            q, x = placement_case(model, d, obs_at)
            for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
                hist = history_numpy(q, x, x0, 17, SEED, 1.0)
                runs.append(((model, obs_at, x0 is None), q, x, x0, SEED, 0, hist, pick_slots(hist["lw"], 65, SEED, int(q.n_pts))[0]))
        for first in (20, 50):
            probs, xs = batch_case(model, d, first)
            for k in range(3):
                hist = history_numpy(probs[k], xs[k], None, 40, SEED_BATCH, 0.5, index=k)
                final = pick_slots(hist["lw"], 17, SEED_BATCH, int(probs[k].n_pts), index=k)[0]
                runs.append(((model, "batch", first, k), probs[k], xs[k], None, SEED_BATCH, k, hist, final))
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    for k, p in enumerate(ps):
        q, x = _fields(p["vgp"]), p["vgp"].initialization()
        hist = history_numpy(q, x, None, 17, SEED_BATCH, 0.5, index=k)
        runs.append((("member", k), q, x, None, SEED_BATCH, k, hist, pick_slots(hist["lw"], 6, SEED_BATCH, int(q.n_pts), index=k)[0]))
    return runs


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p", "quiet_l96d12"])
def test_history_is_the_filter_of_the_paths(tag):
    q, x, x0 = case(tag)
    for start in (None, x0):
        for frac in (0.0, 0.5, 1.0):
            got, want = history_numpy(q, x, start, 17, SEED, frac), particle_paths_numpy(q, x, start, 17, SEED, frac)
            for key in ("lw", "state", "ess", "resampled", "ancestors", "clouds", "obs_t"):
                assert np.array_equal(got[key], want[key]), (tag, frac, key)
            assert got["margins"] == want["margins"]
            assert np.all(np.isfinite(got["hlw"]))
            if int(got["obs_t"][-1]) == int(q.n_pts) - 1:      # (nothing is resampled at the last grid index: the history is the result)
                assert np.array_equal(got["hlw"][-1], got["lw"])


@pytest.mark.parametrize("start", ["given", "drawn"])
@pytest.mark.parametrize("tag", ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p", "quiet_l96d12"])
def test_bit_equalities_of_the_restatement(tag, start):
    """at stride 1 trajectory m passes, bit for bit, through clouds[j][s_j[m]] at every observation and ends in state[s_c[m]]; the table
    differs from the genealogy's where a cloud was resampled"""
    q, x, x0 = case(tag)
    s0 = x0 if start == "given" else None
    differs = False
    for n, k in ((17, 65), (65, 17)):
        for frac in FRACTIONS:
            hist = history(tag, start, n, frac)
            final, _ = pick_slots(hist["lw"], k, SEED, int(q.n_pts))
            table, gaps = backward_slots_numpy(q, x, SEED, hist, final)
            assert len(gaps) == int(hist["resampled"].sum()) and table.min() >= 0 and table.max() < n
            paths = rewalk_backward_numpy(q, x, s0, SEED, table, hist)
            for j, t in enumerate(hist["obs_t"]):
                assert np.array_equal(paths[:, t], hist["clouds"][j][table[j]]), (tag, n, frac, j)
            assert np.array_equal(paths[:, -1], hist["state"][table[-1]]), (tag, n, frac)
            differs = differs or not np.array_equal(table, trace_slots(final, hist["ancestors"], hist["resampled"]))
    # (in one dimension the transition densities of neighbouring particles overlap, so some draw leaves its ancestor; in 12 the
    # successor identifies the particle it was copied from almost surely)
    assert differs or tag not in ("ou_euler", "dw_euler_p")


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p"])
def test_without_resampling_it_is_the_genealogy(tag):
    """ess_fraction 0, and one particle: no draw is made, the table is trace_slots' and the reload changes no bit of rewalk_numpy's paths"""
    q, x, x0 = case(tag)
    for s0 in (None, x0):
        for n, frac in ((17, 0.0), (1, 1.0)):
            hist = history_numpy(q, x, s0, n, SEED, frac)
            final = np.arange(5 if n > 1 else 1) % n      # (one particle, one trajectory: numpy's one-row product is its own routine)
            table, gaps = backward_slots_numpy(q, x, SEED, hist, final)
            assert not gaps and np.array_equal(table, trace_slots(final, hist["ancestors"], hist["resampled"]))
            assert np.array_equal(rewalk_backward_numpy(q, x, s0, SEED, table, hist), rewalk_numpy(q, x, s0, SEED, table))


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------
def test_argmax_on_a_hand_made_table():
    """three candidates: b = (log 1, log 2, log 4) - 700 and Gumbels (0.5, 0.25, -0.5) give the scores (-699.5, -699.0568.., -699.1137..):
    candidate 1 wins with a gap of log 2 + 0.25 - (log 4 - 0.5) = 0.75 - log 2; a tie goes to the smaller slot"""
    b = np.log([1.0, 2.0, 4.0]) - 700.0
    win, gap = argmax_with_gap((b + np.array([0.5, 0.25, -0.5]))[None, :])
    assert win[0] == 1 and abs(gap[0] - (0.75 - np.log(2.0))) <= 1e-12
    win, gap = argmax_with_gap(np.array([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, -1.0, 5.0]]))
    assert np.array_equal(win, [1, 0, 2]) and np.array_equal(gap, [0.0, 0.0, 5.0])
    assert np.array_equal(argmax_with_gap(np.array([[3.0], [4.0]]))[0], [0, 0])


def test_gumbel_pair_convention():
    """slots 2q and 2q + 1 share the Philox call of counter (k, m, p, 0x80000000 | q): the even one takes unit_open(r0, r1), the odd one
    unit_open(r2, r3); the fourth word collides neither with the normals' (below 32) nor with the resamplings' (0xffffffff)"""
    g = gumbels(SEED, 33, [0, 5], 2, 7)
    assert g.shape == (2, 7) and np.all(np.isfinite(g))
    for row, m in enumerate((0, 5)):
        for q in range(4):
            r = philox4x32_10((33, m, 2, 0x80000000 | q), (SEED, 0))
            assert g[row, 2 * q] == -np.log(-np.log(float(unit_open(r[0], r[1]))))
            if 2 * q + 1 < 7:
                assert g[row, 2 * q + 1] == -np.log(-np.log(float(unit_open(r[2], r[3]))))
    assert np.array_equal(gumbels(SEED, 33, [5], 2, 6)[0], g[1, :6])      # (the draws of a slot do not depend on n)
    big = gumbels(3, 1, np.arange(64), 0, 1024)      # Gumbel(0, 1): mean = Euler's constant, variance pi^2 / 6
    assert abs(big.mean() - 0.5772156649) < 0.02 and abs(big.var() - np.pi ** 2 / 6.0) < 0.05


def test_draw_follows_the_backward_kernel():
    """two well-separated candidates with equal weights: a successor that sits on candidate 1's transition mean picks it every time"""
    q, x, _ = case("ou_euler")
    hist = history("ou_euler", "drawn", 17, 1.0)
    j = int(np.flatnonzero(hist["resampled"])[-1])
    fake = dict(hist)
    fake["hlw"] = np.zeros_like(hist["hlw"])
    fake["clouds"] = hist["clouds"].copy()
    fake["clouds"][j] = np.linspace(-40.0, 40.0, 17)[:, None]      # (far apart against R = sqrt(Sigma dt))
    fake["ancestors"] = hist["ancestors"].copy()
    fake["ancestors"][j] = np.arange(17)
    fake["resampled"] = np.zeros_like(hist["resampled"])
    fake["resampled"][j] = 1
    final = np.arange(17)
    table, gaps = backward_slots_numpy(q, x, SEED, fake, final)
    assert np.array_equal(table[j], final) and min(g.min() for g in gaps) > 1.0


# ---- Lorenz-96 cases in which the draw decides ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_draw", TIGHT_RUNS)
@pytest.mark.parametrize("d", TIGHT)
def test_tight_clouds_react_to_the_kernel(d, n, n_draw):
    """what makes the tight cases a test of the Lorenz-96 draw: the table is not the genealogy's, and it changes when the drift of the
    transition means is left out or shifted by one component; and what lets the device's table be compared exactly: every resampling
    decision, threshold and draw keeps its margin"""
    q, x = tight_case(d)
    hist, final, table, gaps = tight_reference(d, n, n_draw)
    assert hist["resampled"][0] == 1 and len(gaps) == int(hist["resampled"].sum())
    assert not np.array_equal(table, trace_slots(final, hist["ancestors"], hist["resampled"]))
    for wrong in (lambda model, theta, z: np.zeros_like(z), lambda model, theta, z: np.roll(model_drift(model, theta, z), 1, axis=1)):
        assert not np.array_equal(backward_slots_numpy(q, x, SEED, hist, final, drift=wrong)[0], table)
    # the decisions ESS < n (1e-6 against a rounding of 1e-13 n), the thresholds of the resamplings and of the pick, the draws
    assert np.all(np.abs(hist["ess"] - n) >= 1e-6) or int(hist["obs_t"][-1]) == int(q.n_pts) - 1
    assert min(hist["margins"]) >= MARGIN and pick_slots(hist["lw"], n_draw, SEED, int(q.n_pts))[1] >= MARGIN
    assert min(float(g.min()) for g in gaps) >= GAP


# ---- the gap condition ---------------------------------------------------------------------------------------------------------------------
def test_gap_condition():
    """a condition on the cases, not a measurement of the device: in every run of tests/test_particle_backward.py the winning score of
    every draw keeps at least 1e-8 (log units) from the runner-up; the device's scores differ from these by about 1e-12"""
    smallest = np.inf
    for run in backward_runs():
        gap = reference(*run)[3]
        smallest = min(smallest, gap)
        assert gap >= GAP, (run, gap)
    print("smallest gap of the fixture runs:", smallest, "over", len(backward_runs()), "runs")
    others = np.inf
    for label, q, x, x0, seed, index, hist, final in other_runs():
        gaps = backward_slots_numpy(q, x, seed, hist, final, index=index)[1]
        gap = min([float(g.min()) for g in gaps], default=np.inf)
        others = min(others, gap)
        assert gap >= GAP, (label, gap)
    print("smallest gap of the placement, batch and member runs:", others)
    tag, n, k, frac, seed = BIG
    gap = reference(tag, "drawn", n, k, frac, seed)[3]
    print("smallest gap of the large run:", gap)
    assert gap >= GAP


# ---- the exact anchor: a linear-Gaussian chain ---------------------------------------------------------------------------------------------
def test_rts_anchor():
    """ou_euler with A_t = theta, 2048 particles, 2048 trajectories, seeds 1 - 8: the seed-mean of the mean and of the variance over the
    backward-simulated trajectories within 4 standard errors of the exact smoothing marginals at grid indices 0, 33, 67 and 100, and in
    every seed more distinct states at index 0 than the genealogy of the same filter run leaves"""
    q, _, _ = case("ou_euler")
    n_pts = int(q.n_pts)
    assert n_pts == 101
    x = np.concatenate((np.full(n_pts, float(q.theta)), np.zeros(n_pts)))      # A_t = theta, b_t = 0: the proposal is the model
    ms, ps = rts_marginals(q)
    at = np.array([0, 33, 67, 100])
    mean, var, smallest = [], [], np.inf
    for seed in range(1, 9):
        hist = history_numpy(q, x, None, 2048, seed, 0.5)
        assert hist["resampled"].sum() >= 2
        final, _ = pick_slots(hist["lw"], 2048, seed, n_pts)
        table, gaps = backward_slots_numpy(q, x, seed, hist, final)
        smallest = min(smallest, min(float(g.min()) for g in gaps))
        draws = rewalk_backward_numpy(q, x, None, seed, table, hist)[:, at, 0]
        mean.append(draws.mean(axis=0))
        var.append(draws.var(axis=0))
        genealogy = np.unique(trace_slots(final, hist["ancestors"], hist["resampled"])[0]).size
        print(f"seed {seed}: distinct states at index 0: backward {np.unique(draws[:, 0]).size}, genealogy {genealogy}")
        assert np.unique(draws[:, 0]).size > genealogy
    mean, var = np.array(mean), np.array(var)
    se_m, se_v = mean.std(axis=0, ddof=1) / np.sqrt(8.0), var.std(axis=0, ddof=1) / np.sqrt(8.0)
    print("exact mean", ms[at], " seed-mean", mean.mean(axis=0), " standard error", se_m)
    print("exact var ", ps[at], " seed-mean", var.mean(axis=0), " standard error", se_v)
    print("smallest top-two gap of the Gumbel scores:", smallest)
    assert np.all(np.abs(mean.mean(axis=0) - ms[at]) <= 4.0 * se_m)
    assert np.all(np.abs(var.mean(axis=0) - ps[at]) <= 4.0 * se_v)


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_keeps_the_method():
    paths = np.arange(3 * 4 * 2, dtype=float).reshape(3, 4, 2)
    slots = np.array([[0, 1, 3], [0, 0, 2], [1, 0, 2], [1, 3, 2]])
    rec = SmoothingPaths([-700.0, -701.0, -702.0, -700.5], paths, slots, 3, 11, [0, 4, 10], method="backward")
    assert rec.method == "backward" and np.array_equal(rec.distinct(), [3, 2, 3, 3])
    assert SmoothingPaths([-700.0, -701.0, -702.0, -700.5], paths, slots, 3, 11, [0, 4, 10]).method == "genealogy"
    with pytest.raises(ValueError, match="method"):
        SmoothingPaths([-700.0, -701.0, -702.0, -700.5], paths, slots, 3, 11, [0, 4, 10], method="rejection")
    assert list(inspect.signature(SmoothingPaths.__init__).parameters)[-1] == "method"
    assert "backward" in SmoothingPaths.__doc__ and "collaps" in SmoothingPaths.__doc__


def test_symbol_and_prototype():
    assert "vgpa_particle_backward_paths" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    protos = {}
    for name in ("vgpa_particle_backward_paths", "vgpa_particle_paths"):
        proto = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name + ": prototype missing"
        protos[name] = " ".join(proto.group(1).split())
    assert protos["vgpa_particle_backward_paths"] == protos["vgpa_particle_paths"]
    assert protos["vgpa_particle_backward_paths"].startswith("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t n_draw, ")


def test_python_surface():
    for owner, new, old in [(va.Context, "particle_backward_paths", "particle_paths"), (va.VarGP, "backward_paths", "particle_paths"),
                            (va.ProblemBatch, "backward_paths", "particle_paths")]:
        fn = getattr(owner, new, None)
        assert callable(fn), owner.__name__
        assert str(inspect.signature(fn)) == str(inspect.signature(getattr(owner, old))), owner.__name__
