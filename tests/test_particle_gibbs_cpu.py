"""
Particle Gibbs with ancestor sampling (vgpa_particle_conditional, VarGP.particle_gibbs): the numpy restatement of the
conditional particle filter, its bit equalities, the margin conditions of the GPU tests, the theta draw against least squares, the
host-side surface and a statistical anchor on a linear chain.

conditional_filter_numpy   test_particle_backward_cpu.history_numpy, from the same pieces (particle_ref), with slot 0 pinned to `ref`: it starts at
                           ref[0], takes the implied increment (ref[k] - ref[k-1]) - dt g in the place of R xi, and is set to ref[k]; the
                           resampling is multinomial for the slots >= 1 and ancestor sampling (Gumbel-max) for slot 0, whose state stays.
conditional_trajectory_numpy   the final slot (pick_slots, one trajectory), trace_slots through the kept ancestors, rewalk_backward_numpy on
                           the run's histories, and the stretches spent in slot 0 overwritten with ref.

The device forms exp / log, the prefix sums and the quadratic form in another order than numpy, so its ancestors are the restatement's
where every ancestor-sampling winner keeps a gap >= GAP from the runner-up and every multinomial threshold u_i S keeps >= BOUNDARY S from
the nearest prefix sum: test_margin_conditions asserts both for every run of tests/test_particle_gibbs.py -- conditions on the cases, not
measurements of the device.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import GibbsChain, path_rows, theta_conditional, theta_draw
from conftest import ROOT
from particle_ref import reset_weights, weight_sums
from test_particle_filter_cpu import MARGIN, SEED, SEED_BATCH, batch_case, case
from test_particle_moments_cpu import rts_marginals
from test_particle_paths_cpu import pick_slots, rewalk_numpy, trace_slots
from test_particle_backward_cpu import argmax_with_gap, history_numpy, rewalk_backward_numpy, tight_case
from test_path_weights_cpu import _sigma_diag, _split, observation_term, obs_model, path_increment, start_term
from test_sample_paths_cpu import em_noise, em_step, model_drift, philox4x32_10, start_cloud, unit_open

GAP = 1e-8            # log units, between the two largest scores of an ancestor draw
BOUNDARY = 1e-9       # of S, between a multinomial threshold and the nearest prefix sum
REF_SEED = 11         # the seed of the particle_paths draw the reference trajectories are
REF_PARTICLES = 17
# the cases of the GPU tests: D = 1 (both one-dimensional models), 3, 12, 17, 40 with a drawn start (the pinned start's initial term), D = 64
# with a given one
GCASES = [("ou_euler", "drawn"), ("dw_euler_p", "drawn"), ("l63_euler_p", "drawn"), ("l96d12_euler_p", "drawn"), ("l96d17_rk4_p", "drawn"),
          ("l96d40_rk4_p", "drawn"), ("l96d64", "given")]
PARTICLES = (1, 17, 65, 300)
GFRACTIONS = (0.0, 0.5, 1.0)
TIGHT = (12, 40)
TIGHT_PARTICLES = 65


def uniforms_multinomial(seed, k, n, index):
    """(n,): u_i = unit_open(r0, r1) of Philox counter (k, i, index, 0xfffffffe); entry 0 is not used"""
    r = philox4x32_10((np.uint64(k), np.arange(n, dtype=np.uint64), np.uint64(index), np.uint64(0xFFFFFFFE)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return unit_open(r[0], r[1])


def gumbels_ancestor(seed, k, n, index):
    """(n,): g_i = -log(-log u_i); u of the slots 2q and 2q + 1 from the one Philox call with counter (k, 0, index, 0x40000000 | q)"""
    pairs = np.arange((n + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((np.uint64(k), np.uint64(0), np.uint64(index), np.uint64(0x40000000) | pairs), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = np.stack((unit_open(r[0], r[1]), unit_open(r[2], r[3])), axis=-1).reshape(-1)[:n]
    return -np.log(-np.log(u))


def bisect_numpy(cum, u):
    """min(#{m: cum_m <= u}, n - 1) per threshold, and the distance of every threshold to the nearest prefix sum"""
    cum, u = np.asarray(cum, dtype=float), np.atleast_1d(np.asarray(u, dtype=float))
    pos = np.searchsorted(cum, u, side="right")
    near = np.min(np.abs(u[:, None] - cum[None, :]), axis=1)
    return np.minimum(pos, cum.size - 1), near


def ancestor_draw(lw, quad, g, transition=True):
    """(the smallest i that attains max (b_i + g_i), the gap to the runner-up): b = lw - quad / 2 (transition=False: b = lw, the mutant)"""
    b = lw - 0.5 * quad if transition else lw
    win, gap = argmax_with_gap((b + g)[None, :])
    return int(win[0]), float(gap[0])


def pinned_draw(problem, theta, rdiag, cloud, lw, ref, k, seed, index=0, transition=True, drift=model_drift, divisor=None, target=None,
                weights=None, swap_halves=False, limit=None):
    """(winner, gap) of the pinned slot's ancestor draw at grid index k on the cloud (n, D) with the log-weights lw (n,) before the reset:
    x~ = ref[k + 1], mu_i = x_i + dt f(x_i; theta), quad_i = sum_d ((x~_d - mu_i,d) / R_dd)^2, ancestor_draw on lw, quad and the Gumbels of
    the cut.  With the defaults this is conditional_filter_numpy's own draw, operation for operation.  The other arguments are the hooks of
    the mutants of test_particle_ancestor_cpu: drift(model, theta, cloud) in the model drift's place, divisor(rdiag) -> the divisors used,
    target(ref, k) -> the x~ used, weights(lw) -> the log-weights used, swap_halves: candidates 2q and 2q + 1 take each other's half of
    their Philox call, limit: candidates >= limit are not scored."""
    n, dt = lw.size, float(problem.dt)
    mu = cloud + dt * drift(problem.model, theta, cloud)
    xt = ref[k + 1] if target is None else target(ref, k)
    div = rdiag if divisor is None else divisor(rdiag)
    quad = np.sum(((xt[None, :] - mu) / div[None, :]) ** 2, axis=1)
    g = gumbels_ancestor(seed, k, n, index)
    if swap_halves:
        g = gumbels_ancestor(seed, k, n + (n & 1), index).reshape(-1, 2)[:, ::-1].reshape(-1)[:n]
    used = lw if weights is None else weights(lw)
    if limit is not None and limit < n:
        used = np.where(np.arange(n) < limit, used, -np.inf)
    return ancestor_draw(used, quad, g, transition)


def conditional_filter_numpy(problem, x, x0, ref, n, seed, ess_fraction, index=0, transition=True, eta_dt=None):
    """One problem's conditional filter with counter word `index`.  Returns history_numpy's dict (ancestors[j][0]: the ancestor-sampled one)
    and gaps (of the ancestor draws), margins (of the multinomial thresholds, relative to S).  eta_dt: the factor in dt's place inside the
    implied increment of the pinned slot (a mutant's; None: dt)."""
    d, n_pts, dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
    sigma = _sigma_diag(problem)
    isg, fac = 1.0 / sigma.diagonal(), np.linalg.cholesky(sigma * dt)
    rdiag = fac.diagonal()
    lin_a, off_b = _split(problem, x)
    theta = np.asarray(problem.theta, dtype=float)
    obs_t, obs_y, q, const = obs_model(problem)
    at = {int(t): j for j, t in enumerate(obs_t)}
    slots = np.arange(n)
    ref = np.asarray(ref, dtype=float).reshape(n_pts, d)
    state = start_cloud(problem, x0, seed, slots, index)
    state[0] = ref[0]
    m = obs_t.size
    out = dict(ess=np.zeros(m), resampled=np.zeros(m, dtype=np.int64), ancestors=np.full((m, n), -1, dtype=np.int64),
               clouds=np.full((m, n, d), np.nan), hlw=np.full((m, n), np.nan), margins=[], gaps=[])
    lw = start_term(problem, state, x0) - const
    for k in range(n_pts):
        if k > 0:
            g = -(state @ lin_a[k - 1].T) + off_b[k - 1]
            dd = g - model_drift(problem.model, theta, state)
            eta = em_noise(seed, k, slots, index, fac)
            eta[0] = (ref[k] - state[0]) - (dt if eta_dt is None else eta_dt) * g[0]
            lw = lw + path_increment(dd, eta, isg, dt)
            state = em_step(state, dt, g, eta)
            state[0] = ref[k]
        if k not in at:
            continue
        j = at[k]
        lw = lw + observation_term(obs_y[j], state, q)
        top, _, cum, total, ess = weight_sums(lw)
        out["ess"][j], out["clouds"][j], out["ancestors"][j], out["hlw"][j] = ess, state, slots, lw
        if ess < ess_fraction * n and k < n_pts - 1:
            anc, near = bisect_numpy(cum, uniforms_multinomial(seed, k, n, index) * total)
            out["margins"].append(float(near[1:].min() / total) if n > 1 else np.inf)
            win, gap = pinned_draw(problem, theta, rdiag, state, lw, ref, k, seed, index, transition)
            out["gaps"].append(gap)
            hist = anc.copy()
            hist[0], anc[0] = win, 0          # (the pinned slot keeps its state; its ancestor goes into the history alone)
            out["resampled"][j], out["ancestors"][j] = 1, hist
            state, lw = state[anc], reset_weights(top, total, n)
    out.update(lw=lw, state=state, obs_t=np.asarray(obs_t, dtype=np.int64))
    return out


def conditional_trajectory_numpy(problem, x, x0, ref, seed, hist, index=0, table=None, side="left"):
    """(trajectory (Np, D), table (M + 1,), the pick's margin): the final slot drawn from the final weights, traced through the kept
    ancestors, walked by the backward walk on the run's histories; where the table says slot 0, the reference.  side: "left" counts the
    observations before k (t_m < k: the stretch of grid index k); "right" is the mutant t_m <= k of the fill."""
    n_pts = int(problem.n_pts)
    final, margin = pick_slots(hist["lw"], 1, seed, n_pts, index=index)
    if table is None:
        table = trace_slots(final, hist["ancestors"], hist["resampled"])
    table = np.asarray(table, dtype=np.int64).reshape(-1, 1)
    # (as many copies of the one trajectory as the filter has particles: numpy's matrix product rounds by the shape of its operands)
    path = rewalk_backward_numpy(problem, x, x0, seed, np.repeat(table, hist["lw"].size, axis=1), hist, index=index)[0]
    ref = np.asarray(ref, dtype=float).reshape(path.shape)
    stretch = np.searchsorted(hist["obs_t"], np.arange(n_pts), side=side)
    mine = table[stretch, 0] == 0
    path[mine] = ref[mine]
    return path, table[:, 0], margin


@functools.lru_cache(maxsize=None)
def reference_path(tag, start):
    """the reference trajectory of a case: one drawn trajectory of the particle_paths restatement at REF_SEED (read-only)"""
    q, x, x0 = case(tag)
    s0 = x0 if start == "given" else None
    hist = history_numpy(q, x, s0, REF_PARTICLES, REF_SEED, 0.5)
    final, _ = pick_slots(hist["lw"], 1, REF_SEED, int(q.n_pts))
    path = rewalk_numpy(q, x, s0, REF_SEED, trace_slots(final, hist["ancestors"], hist["resampled"]))[0]
    path.setflags(write=False)
    return path


@functools.lru_cache(maxsize=None)
def reference(tag, start, n, ess_fraction, seed=SEED):
    """(history, trajectory, table, pick margin) of a run of tests/test_particle_gibbs.py, computed once per process (read-only)"""
    q, x, x0 = case(tag)
    s0 = x0 if start == "given" else None
    ref = reference_path(tag, start)
    hist = conditional_filter_numpy(q, x, s0, ref, n, seed, ess_fraction)
    return (hist,) + conditional_trajectory_numpy(q, x, s0, ref, seed, hist)


@functools.lru_cache(maxsize=None)
def tight_reference_path(d):
    q, x = tight_case(d)
    hist = history_numpy(q, x, None, REF_PARTICLES, REF_SEED, 1.0)
    final, _ = pick_slots(hist["lw"], 1, REF_SEED, int(q.n_pts))
    path = rewalk_numpy(q, x, None, REF_SEED, trace_slots(final, hist["ancestors"], hist["resampled"]))[0]
    path.setflags(write=False)
    return path


@functools.lru_cache(maxsize=None)
def tight_reference(d, transition=True):
    q, x = tight_case(d)
    ref = tight_reference_path(d)
    hist = conditional_filter_numpy(q, x, None, ref, TIGHT_PARTICLES, SEED, 1.0, transition=transition)
    return (hist,) + conditional_trajectory_numpy(q, x, None, ref, SEED, hist)


@functools.lru_cache(maxsize=None)
def batch_reference(model, d, first):
    """per problem k of test_particle_filter_cpu.batch_case: (reference trajectory, history, trajectory, table, pick margin) of the runs
    with 40 particles, SEED_BATCH, ess_fraction 0.5 and counter word k; the references are drawn at SEED_BATCH + 1"""
    probs, xs = batch_case(model, d, first)
    out = []
    for k, q in enumerate(probs):
        h0 = history_numpy(q, xs[k], None, REF_PARTICLES, SEED_BATCH + 1, 0.5, index=k)
        final, _ = pick_slots(h0["lw"], 1, SEED_BATCH + 1, int(q.n_pts), index=k)
        ref = rewalk_numpy(q, xs[k], None, SEED_BATCH + 1, trace_slots(final, h0["ancestors"], h0["resampled"]), index=k)[0]
        hist = conditional_filter_numpy(q, xs[k], None, ref, 40, SEED_BATCH, 0.5, index=k)
        out.append((ref, hist) + conditional_trajectory_numpy(q, xs[k], None, ref, SEED_BATCH, hist, index=k))
    return out


def gibbs_runs():
    """every (case, start, particles, ess_fraction) tests/test_particle_gibbs.py runs on the fixtures; the seed is SEED"""
    return [(tag, start, n, frac) for tag, start in GCASES for n in PARTICLES for frac in GFRACTIONS]


def check_identities(q, hist, path, table, ref):
    """the four bit identities of vgpa_hip.h on one run"""
    n_pts = int(q.n_pts)
    stretch = np.searchsorted(hist["obs_t"], np.arange(n_pts), side="left")
    mine = table[stretch] == 0
    assert np.array_equal(path[mine], np.asarray(ref)[mine])
    for j, t in enumerate(hist["obs_t"]):
        assert np.array_equal(path[int(t)], hist["clouds"][j][table[j]]), j
        assert np.array_equal(hist["clouds"][j][0], np.asarray(ref)[int(t)]), j
    assert np.array_equal(path[-1], hist["state"][table[-1]])


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,start", [("ou_euler", "drawn"), ("l63_euler_p", "given"), ("l96d12_euler_p", "drawn")])
def test_without_resampling_the_other_slots_are_the_filters(tag, start):
    q, x, x0 = case(tag)
    s0 = x0 if start == "given" else None
    ref = reference_path(tag, start)
    got, want = conditional_filter_numpy(q, x, s0, ref, 17, SEED, 0.0), history_numpy(q, x, s0, 17, SEED, 0.0)
    assert np.array_equal(got["state"][1:], want["state"][1:]) and np.array_equal(got["lw"][1:], want["lw"][1:])
    assert np.array_equal(got["clouds"][:, 1:], want["clouds"][:, 1:]) and not got["resampled"].any() and not got["gaps"]
    assert np.array_equal(got["state"][0], ref[-1]) and np.array_equal(got["clouds"][:, 0], ref[got["obs_t"]])


@pytest.mark.parametrize("tag,start", GCASES[:4])
def test_identities_of_the_restatement(tag, start):
    q = case(tag)[0]
    ref = reference_path(tag, start)
    moved = False
    for n in (1, 17, 65):
        for frac in GFRACTIONS:
            hist, path, table, _ = reference(tag, start, n, frac)
            check_identities(q, hist, path, table, ref)
            assert table.min() >= 0 and table.max() < n
            if n == 1:
                assert np.array_equal(path, ref) and not hist["resampled"].any()
            moved = moved or not np.array_equal(path, ref)
    # (in 12 dimensions the fixture's reference, a surviving lineage of a filter, outweighs 65 fresh particles in every run: the sweep
    # returns it; the tight cases are where Lorenz-96 moves)
    assert moved or int(q.dim_d) > 3


def test_the_pinned_weight_is_the_weight_of_the_reference():
    """slot 0's log-weight without resampling is the importance weight of the reference path: the implied increments reproduce it, so a
    reference that IS slot 5's own path of the plain filter gets slot 5's weight (to rounding: eta* is recomputed from the states)"""
    q, x, _ = case("l63_euler_p")
    from test_particle_paths_cpu import particle_paths_numpy
    fwd = particle_paths_numpy(q, x, None, 8, SEED, 0.0)
    got = conditional_filter_numpy(q, x, None, fwd["paths"][5], 8, SEED, 0.0)
    assert abs(got["lw"][0] - fwd["lw"][5]) <= 1e-9 * abs(fwd["lw"][5])


# ---- ties and boundaries -------------------------------------------------------------------------------------------------------------------
def test_ancestor_draw_on_a_hand_made_table():
    """three candidates; a tie goes to the smaller slot; without the transition term the heaviest candidate wins"""
    lw = np.log([1.0, 2.0, 4.0]) - 700.0
    g = np.array([0.5, 0.25, -0.5])
    win, gap = ancestor_draw(lw, np.zeros(3), g)
    assert win == 1 and abs(gap - (0.75 - np.log(2.0))) <= 1e-12
    assert ancestor_draw(np.zeros(3), np.zeros(3), np.array([1.0, 3.0, 3.0]))[0] == 1 and ancestor_draw(np.zeros(3), np.zeros(3), np.array([1.0, 3.0, 3.0]))[1] == 0.0
    assert ancestor_draw(np.zeros(3), np.zeros(3), np.zeros(3)) == (0, 0.0)
    assert ancestor_draw(lw, np.array([0.0, 40.0, 40.0]), g)[0] == 0 and ancestor_draw(lw, np.array([0.0, 40.0, 40.0]), g, transition=False)[0] == 1
    assert ancestor_draw(np.array([-3.0]), np.array([2.0]), np.array([0.1]))[0] == 0


def test_multinomial_bisection_on_a_hand_made_table():
    cum = np.array([0.25, 0.75, 1.5, 2.5])
    anc, near = bisect_numpy(cum, [0.0, 0.2, 0.25, 0.74, 0.75, 1.4999, 2.4999, 2.5])
    assert np.array_equal(anc, [0, 0, 1, 1, 2, 2, 3, 3])      # (a threshold on a boundary belongs to the slot above; u = S is clipped)
    assert np.allclose(near, [0.25, 0.05, 0.0, 0.01, 0.0, 1e-4, 1e-4, 0.0], atol=1e-12)
    assert np.array_equal(bisect_numpy([1.0], [0.3, 1.0])[0], [0, 0])
    u = uniforms_multinomial(SEED, 33, 6, 2)
    r = philox4x32_10((33, 4, 2, 0xFFFFFFFE), (SEED, 0))
    assert u[4] == float(unit_open(r[0], r[1])) and np.all((u > 0.0) & (u < 1.0))
    g = gumbels_ancestor(SEED, 33, 5, 2)
    r = philox4x32_10((33, 0, 2, 0x40000001), (SEED, 0))
    assert g[2] == -np.log(-np.log(float(unit_open(r[0], r[1])))) and g[3] == -np.log(-np.log(float(unit_open(r[2], r[3]))))


# ---- the margin conditions -------------------------------------------------------------------------------------------------------------------
def test_margin_conditions():
    """conditions on the cases, not measurements of the device: every ancestor draw keeps >= 1e-8 between winner and runner-up, every
    multinomial threshold >= 1e-9 S from the nearest prefix sum, the pick of the final slot >= 1e-7 S"""
    gap, margin, pick, resampled = np.inf, np.inf, np.inf, 0
    for tag, start, n, frac in gibbs_runs():
        hist, _, _, pm = reference(tag, start, n, frac)
        gap, margin, pick = min([gap] + hist["gaps"]), min([margin] + hist["margins"]), min(pick, pm)
        resampled += int(hist["resampled"].sum())
        assert min(hist["gaps"], default=np.inf) >= GAP and min(hist["margins"], default=np.inf) >= BOUNDARY and pm >= MARGIN, (tag, start, n, frac)
    for d in TIGHT:
        hist, _, _, pm = tight_reference(d)
        assert min(hist["gaps"]) >= GAP and min(hist["margins"]) >= BOUNDARY and pm >= MARGIN, d
    for model, d in (("L96", 12), ("L63", 3)):
        for first in (20, 50):
            for k, (_, hist, _, _, pm) in enumerate(batch_reference(model, d, first)):
                assert min(hist["gaps"], default=np.inf) >= GAP and min(hist["margins"], default=np.inf) >= BOUNDARY and pm >= MARGIN, (model, first, k)
    print("smallest gap", gap, "smallest margin", margin, "smallest pick margin", pick, "resampled cuts", resampled)
    assert resampled > 100


# ---- the mutant ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", TIGHT)
def test_tight_clouds_react_to_the_transition_term(d):
    """on the tight Lorenz-96 clouds the pinned slot's ancestor is not always itself, and it changes when the transition density is
    dropped from the score: the draw depends on x~, the drift and 1 / R"""
    hist, path, table, _ = tight_reference(d)
    mutant = tight_reference(d, transition=False)[0]
    cuts = np.flatnonzero(hist["resampled"])
    assert cuts.size and np.any(hist["ancestors"][cuts, 0] != 0)
    first = cuts[0]      # (the histories agree up to the first resampled cut: the mutant's draw there sees the same cloud)
    assert np.array_equal(hist["clouds"][first], mutant["clouds"][first]) and hist["ancestors"][first, 0] != mutant["ancestors"][first, 0]
    check_identities(tight_case(d)[0], hist, path, table, tight_reference_path(d))


# ---- the theta draw --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,model", [("ou_euler", "OU"), ("dw_euler_p", "DW"), ("l63_euler_p", "L63"), ("l96d12_euler_p", "L96")])
def test_theta_conditional_is_weighted_least_squares(tag, model):
    """x_k - x_{k-1} - dt f0(x_{k-1}) = dt Phi theta + noise of covariance Sigma dt: the conditional mean is the weighted least-squares
    solution of the stacked rows, the precision its normal matrix, to 1e-12 relative"""
    q, x, _ = case(tag)
    path = rewalk_numpy(q, x, None, REF_SEED, np.zeros((np.asarray(q.obs_t).size + 1, 1), dtype=np.int64))[0]      # (one path of the posterior process)
    d, dt = int(q.dim_d), float(q.dt)
    theta = np.atleast_1d(np.asarray(q.theta, dtype=float))
    sg = _sigma_diag(q).diagonal()
    mean, prec = theta_conditional(model, theta, path, dt, sg)
    xs = path[:-1]
    zero = np.zeros_like(theta)
    f0 = model_drift(q.model, zero if theta.size > 1 else 0.0, xs)
    cols = []
    for a in range(theta.size):
        e = zero.copy()
        e[a] = 1.0
        cols.append((model_drift(q.model, e if theta.size > 1 else 1.0, xs) - f0).ravel())
    wgt = np.tile(1.0 / np.sqrt(sg * dt), xs.shape[0])
    design = dt * np.stack(cols, axis=1) * wgt[:, None]
    target = (path[1:] - xs - dt * f0).ravel() * wgt
    sol = np.linalg.lstsq(design, target, rcond=None)[0]
    info = np.diag(design.T @ design)
    assert np.all(np.abs(mean - sol) <= 1e-12 * np.abs(sol)), (mean, sol)
    assert np.all(np.abs(prec - info) <= 1e-12 * info), (prec, info)
    # a prior: precision adds, the mean is the precision-weighted one; the draw's keying
    pm, pl = theta + 1.0, 0.5 * prec
    m2, p2 = theta_conditional(model, theta, path, dt, sg, (pm, pl))
    assert np.allclose(p2, 1.5 * prec, rtol=1e-14) and np.allclose(m2, (prec * mean + pl * pm) / p2, rtol=1e-12)
    z = np.random.Generator(np.random.PCG64([5, 3, 2])).standard_normal(theta.shape)
    assert np.array_equal(theta_draw(mean, prec, 5, 3, 2), mean + z / np.sqrt(prec))
    assert not np.array_equal(theta_draw(mean, prec, 5, 3, 2), theta_draw(mean, prec, 5, 4, 2))
    rows = path_rows(model, theta, path, dt)
    assert rows.shape == (3, d) and np.all(rows[0] > 0.0) and np.all(rows[2] > 0.0)


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record():
    paths = np.arange(4 * 5 * 2, dtype=float).reshape(4, 5, 2) ** 1.5
    theta = np.arange(14, dtype=float).reshape(7, 2)
    rec = GibbsChain(theta, paths, [1, 2, 4, 5], [0.0, 1.0, 0.5, 0.25, 1.0, 1.0], first=paths[0])
    assert len(rec) == 6 and np.array_equal(rec.mean(), paths.mean(axis=0)) and np.array_equal(rec.var(2), paths[1:].var(axis=0))
    assert np.array_equal(rec.mean(5), paths[3]) and np.array_equal(rec.theta_mean(), theta[1:].mean(axis=0))
    assert np.array_equal(rec.theta_mean(4), theta[5:].mean(axis=0)) and np.array_equal(rec.theta_var(4), theta[5:].var(axis=0))
    one = GibbsChain(theta[:3, :1], paths[:2, :, :1], [0, 1], [1.0, 1.0], single_dim=True)
    assert one.paths.shape == (2, 5) and one.mean().shape == (5,)
    for bad in (lambda: GibbsChain(theta, paths, [1, 2, 4], [0.0] * 6), lambda: GibbsChain(theta, paths, [1, 2, 4, 6], [0.0] * 6),
                lambda: GibbsChain(theta, paths, [1, 2, 4, 5], [0.0] * 5), lambda: GibbsChain(theta, paths, [2, 1, 4, 5], [0.0] * 6),
                lambda: rec.mean(6)):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_conditional" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_conditional\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, const double* ref, int32_t n_paths, uint64_t seed, "
                    "double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, "
                    "double* trajectory, int32_t* slots_or_null, double* ess_or_null, int32_t* resampled_or_null, int32_t* ancestors_or_null, "
                    "double* clouds_or_null")


def test_python_surface():
    sig = inspect.signature(va.Context.particle_conditional).parameters
    assert list(sig)[1:] == ["ref", "n_paths", "seed", "ess_fraction", "x", "x0", "prior", "history"]
    assert sig["ess_fraction"].default == 0.5 and sig["history"].default is False
    for owner in (va.VarGP, va.ProblemBatch):
        sig = inspect.signature(owner.particle_gibbs).parameters
        assert list(sig)[1:9] == ["n_paths", "seed", "iters", "burn", "thin", "ess_fraction", "sample_theta", "theta_prior"], owner.__name__
        assert (sig["burn"].default, sig["thin"].default, sig["ess_fraction"].default, sig["sample_theta"].default, sig["theta_prior"].default) == \
            (0, 1, 0.5, True, None)
    assert va.GibbsChain is GibbsChain and "GibbsChain" in va.__all__
    for name in ("mean", "var", "theta_mean", "theta_var"):
        assert "burn" in inspect.signature(getattr(GibbsChain, name)).parameters
    assert "exact for the Euler-discretised" in " ".join(va.ProblemBatch.particle_gibbs.__doc__.split())


# ---- the statistical anchor, on the restatement --------------------------------------------------------------------------------------------
ANCHOR_AT = np.array([0, 33, 67, 100])
ANCHOR_MEAN = np.array([0.1784, -0.3182, -0.6983, -0.5012])      # the exact RTS values quoted in DESIGN.md s.4.17
ANCHOR_VAR = np.array([0.2368, 0.03410, 0.03379, 0.2123])


def test_rts_anchor():
    """ou_euler with A_t = theta, b_t = 0 (the proposal is the model), 16 particles, theta fixed, 8 seeds x (30 burn-in + 100 kept)
    iterations of the restatement (cut from 50 + 400, which pass as well, to keep the test under a minute): the seed-mean of the chain mean and of the chain variance of x at grid indices 0, 33, 67 and 100 within
    4 standard errors of the exact smoothing marginals.
    Observed z-scores at indices 0, 33, 67, 100: of the chain mean 0.69, -0.01, -0.38, -1.09; of the chain variance -1.57, -0.70, -2.29, 0.63
    (55 s on one core; with 50 + 400 iterations, 156 s: -1.03, 0.06, 0.39, -0.04 and -2.89, -0.24, -1.66, 1.26).  About 79 % of the
    grid points are renewed per sweep."""
    q, _, _ = case("ou_euler")
    n_pts = int(q.n_pts)
    assert n_pts == 101
    ms, ps = rts_marginals(q)
    assert np.allclose(ms[ANCHOR_AT], ANCHOR_MEAN, atol=5e-5) and np.allclose(ps[ANCHOR_AT], ANCHOR_VAR, rtol=2e-3)
    x = np.concatenate((np.full(n_pts, float(q.theta)), np.zeros(n_pts)))
    mean, var, moved = [], [], []
    for seed in range(1, 9):
        hist = history_numpy(q, x, None, 16, seed, 0.5)
        final, _ = pick_slots(hist["lw"], 1, seed, n_pts)
        ref = rewalk_numpy(q, x, None, seed, trace_slots(final, hist["ancestors"], hist["resampled"]))[0]
        kept = []
        for it in range(130):
            run = 1000 * seed + it
            h = conditional_filter_numpy(q, x, None, ref, 16, run, 0.5)
            new = conditional_trajectory_numpy(q, x, None, ref, run, h)[0]
            if it >= 30:
                kept.append(new[ANCHOR_AT, 0])
                moved.append(float(np.mean(new[:, 0] != ref[:, 0])))
            ref = new
        kept = np.array(kept)
        mean.append(kept.mean(axis=0))
        var.append(kept.var(axis=0))
    mean, var = np.array(mean), np.array(var)
    se_m, se_v = mean.std(axis=0, ddof=1) / np.sqrt(8.0), var.std(axis=0, ddof=1) / np.sqrt(8.0)
    z_m, z_v = (mean.mean(axis=0) - ms[ANCHOR_AT]) / se_m, (var.mean(axis=0) - ps[ANCHOR_AT]) / se_v
    print("z-scores of the chain mean", z_m, "of the chain variance", z_v, "mean share of the trajectory renewed per sweep", np.mean(moved))
    assert np.all(np.abs(z_m) <= 4.0) and np.all(np.abs(z_v) <= 4.0)
