"""
The marginal backward smoother (vgpa_particle_backward_moments) without a device: the numpy restatement of its weight
table, the longdouble twin, the floor of the rounding bound, what the restatement must satisfy, the exact anchor on a linear chain, the
conditions of the GPU tests' cases and the host-side surface.  tests/test_particle_backward_moments.py (GPU) imports everything from here.

backward_step              one cut: W^j from W^{j+1} and the histories of test_particle_backward_cpu.history_numpy (or the device's own), as
                           vgpa_hip.h states it, in the number type T -- np.float64 (the oracle) or np.longdouble (the reference) -- with
                           the hooks of backward_slots_numpy (drift, divisor, target) and one more for the hlw term
backward_weights_numpy     the table (M + 1, n): row M the normalised final weights, row j < M a copy or backward_step; its ESS
backward_weights_longdouble  the twin
replay_numpy               x_i(k) of every slot and grid index: particle_ref.visited_states through the stored ancestors
smoothing_moments          M1, M2 and sum W |x| on the grid from a table and the replay

The bound, per cut (one recursion step, as in test_particle_rounding_cpu): with W^{j+1} given, the row under test against the longdouble
step, in units of the floor,

    err_k <= 32 max(err_o, 1)          err_o: the float64 step on the same inputs

The floor of entry i is 2^-53 ((4 + levels(D)) Bmax + 2 + 2 levels(n)) max(W^j_i, 2^-53 max_i W^j_i):
  Bmax       the largest |hlw_i| + q_{s,i} / 2 (q the quadratic form; it is |b_{s,i}| wherever hlw_i <= 0, and never below it) among the
             terms with P_{s,i} > 2^-53 -- a term below that changes no row sum and no weight by a rounding.  An absolute error delta in
             b_{s,i} or in max_i b is a relative error delta in P_{s,i}; the roundings at that size: the scaling by 1 / R and the square of
             every term of q (2), q's own additions as a balanced tree (levels(D)), the subtraction hlw - q / 2 (1), the subtraction of the
             row's maximum (1)
  2 + 2 levels(n)  the division by the row's sum and the product W_s P_{s,i} (2), the two sums of n terms (the row's, the column's)
  2^-53 max W  an entry that small adds less than one rounding of the largest term to any sum of W x: its own relative error does not count
Bmax is computed by the longdouble step itself and printed (test_floor_is_reported); nothing about it is fixed in advance.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import BackwardSmoothingMoments, _weights_of, descendant_weights
from conftest import ROOT
from particle_ref import visited_states
from test_gpu_edge_cases import make_problem
from test_particle_backward_cpu import BCASES, TIGHT, TIGHT_RUNS, history, history_numpy, tight_case
from test_particle_filter_cpu import FRACTIONS, PLACEMENTS, SEED, SEED_BATCH, batch_case, case, placement_case
from test_particle_moments_cpu import particle_moments_numpy, rts_marginals
from test_particle_paths_cpu import DRAWN
from test_particle_rounding_cpu import FACTOR, UNIT, errors, ratio, within
from test_path_weights_cpu import FIXTURES, _sigma_diag, _split
from test_sample_paths_cpu import model_drift

LD = np.longdouble
F64 = np.float64
# particles per problem of the GPU tests: DRAWN's (1, 17, 65, 300) and 257 -- one candidate; a partial 16-successor block and a partial wave;
# a wave and one more; a 256-candidate tile and one more; a ragged second tile
SIZES = tuple(sorted({n for n, _ in DRAWN} | {17, 65, 257, 300}))
LONG = ("OU", "DW", "L63")      # 20 observations at the grid indices 10, 20, ..., 200 (dt 0.01): the clouds overlap, 16 - 19 of them resampled
LONG_N = 128
MUTANT = 1.0 + 2.0 ** -30


class Bmax(float):
    """the largest |hlw_i| + q_{s,i} / 2 of a cut among the terms with P > 2^-53, with the cut's leak beside it"""

    def __new__(cls, value, leak, rho2=float("nan")):
        self = super().__new__(cls, value)
        self.leak, self.rho2 = leak, rho2
        return self


def backward_step(problem, x, seed, hist, j, w_next, index=0, T=F64, drift=None, divisor=None, target=None, hlw=None, gram=False):
    """(W^j (n,), Bmax): the cut at observation j of a problem whose cloud was resampled there.  hist: clouds (M, n, D), ancestors (M, n),
    hlw (M, n), obs_t.  drift(model, theta, cloud) -> f, divisor(rdiag), target(z, x~), hlw(hlw_j): the mutants' hooks.  Bmax is a float
    that also carries .leak = max_s (1 - P_{s, anc_j[s]}): how far P is from the genealogy's indicator, and .rho2: the largest
    |(x~_s - c) / R|^2 or |(mu_i - c) / R|^2, c the cloud's mean.  gram: the quadratic form as (|a_s|^2 + |m_i|^2) - 2 <a_s, m_i> with
    a = (x~ - c) / R and m = (mu - c) / R, the form of the device's matrix-core kernels (D >= 5), in place of the sum of squared differences."""
    d, dt = int(problem.dim_d), float(problem.dt)
    rdiag = np.linalg.cholesky(_sigma_diag(problem) * dt).diagonal()
    lin_a, off_b = _split(problem, x)
    theta = np.asarray(problem.theta, dtype=float)
    k = int(hist["obs_t"][j])
    cloud = np.asarray(hist["clouds"][j], dtype=T).reshape(-1, d)
    n = cloud.shape[0]
    z = cloud[np.asarray(hist["ancestors"][j], dtype=np.int64)]
    g, _ = xr.posterior_drift(lin_a[k], off_b[k], z, T)
    xi, _ = xr.normals(seed, k + 1, np.arange(n), index, d, T)
    xt = (z + T(dt) * g) + xi * np.asarray(rdiag, dtype=T)
    if target is not None:
        xt = np.asarray(target(z, xt), dtype=T)
    div = np.asarray(rdiag if divisor is None else divisor(rdiag), dtype=T)
    f = xr.model_drift(problem.model, theta, cloud, T)[0] if drift is None else np.asarray(drift(problem.model, theta, np.asarray(cloud, dtype=F64)), dtype=T)
    mu = cloud + T(dt) * np.reshape(f, cloud.shape)
    lwj = np.asarray(hist["hlw"][j] if hlw is None else hlw(hist["hlw"][j]), dtype=T)
    wn = np.asarray(w_next, dtype=T)
    p = np.empty((n, n), dtype=T)
    bmax = 0.0
    anc = np.asarray(hist["ancestors"][j], dtype=np.int64)
    block = max(1, (1 << 21) // (n * d))      # successors at a time: at most 2^21 entries of (successor, candidate, component)
    cen = xr._sum(cloud, 0) / n
    ga, gm = (xt - cen) / div, (mu - cen) / div
    na, nm = xr._sum(ga * ga, 1), xr._sum(gm * gm, 1)
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        if gram:
            half = ((na[lo:hi, None] + nm[None, :]) - 2 * (ga[lo:hi] @ gm.T)) / 2
        else:
            v = (xt[lo:hi, None, :] - mu[None, :, :]) / div
            half = xr._sum(v * v, 2) / 2
        b = lwj[None, :] - half
        e = np.exp(b - b.max(axis=1, keepdims=True))
        p[lo:hi] = e / xr._sum(e, 1)[:, None]
        sel = p[lo:hi] > UNIT
        bmax = max(bmax, float((np.abs(lwj)[None, :] + half)[sel].max()))
    return xr._sum(wn[:, None] * p, 0), Bmax(bmax, float(np.max(1 - p[np.arange(n), anc])), float(max(na.max(), nm.max())))


def backward_weights_numpy(problem, x, seed, hist, index=0, T=F64, **hooks):
    """(table (M + 1, n), smoothing_ess (M + 1,), Bmax (M,): nan where the cloud was carried on)"""
    m, n = int(np.asarray(hist["obs_t"]).size), int(np.asarray(hist["lw"]).size)
    table, bmax = np.empty((m + 1, n), dtype=T), np.full(m, np.nan)
    if T is F64:
        table[m] = _weights_of(np.asarray(hist["lw"], dtype=float))
    else:
        lw = np.asarray(hist["lw"], dtype=T)
        w = np.exp(lw - lw.max())
        table[m] = w / xr._sum(w, 0)
    for j in range(m - 1, -1, -1):
        if hist["resampled"][j]:
            table[j], bmax[j] = backward_step(problem, x, seed, hist, j, table[j + 1], index, T, **hooks)
        else:
            table[j] = table[j + 1]
    return table, 1.0 / np.sum(table * table, axis=1), bmax


backward_weights_longdouble = functools.partial(backward_weights_numpy, T=LD)


def floor_size(w_ext, bmax, n, d):
    """the floor of a row in units of 2^-53, entry by entry (the module's docstring)"""
    w = np.asarray(w_ext, dtype=LD)
    return ((4 + xr.levels(d)) * LD(bmax) + 2 + 2 * xr.levels(n)) * np.maximum(w, LD(UNIT) * w.max())


def step_errors(problem, x, seed, hist, j, w_next, got, index=0):
    """(e_k, e_o, Bmax) of a row `got` for the cut j against the longdouble step from w_next, the float64 step as the oracle"""
    ext, bmax = backward_step(problem, x, seed, hist, j, w_next, index, LD)
    orc, _ = backward_step(problem, x, seed, hist, j, w_next, index, F64)
    e_k, e_o = errors(got, ext, orc, floor_size(ext, bmax, ext.size, int(problem.dim_d)))
    return e_k, e_o, bmax


def replay_numpy(problem, x, x0, seed, hist, index=0):
    """(Np, n, D): the state of slot i as the walk arrives at k, before a resampling decision at k -- history_numpy's walk with the stored
    ancestors (the identity where the cloud was carried on) in place of the decisions"""
    gathers = {int(t): np.asarray(hist["ancestors"][j], dtype=np.int64) for j, t in enumerate(hist["obs_t"])}
    return visited_states(problem, x, x0, seed, int(np.asarray(hist["lw"]).size), gathers, index)[0]


def smoothing_moments(table, states, obs_t, stride=1):
    """(M1, M2, A1), each (n_keep, D): sum_i W^{j(k)}_i x_i(k), ... x_i(k)^2, ... |x_i(k)| at k = 0, stride, ...; j(k) = #{observations before k}"""
    grid = np.arange(0, states.shape[0], stride)
    w = np.asarray(table, dtype=float)[np.searchsorted(np.asarray(obs_t), grid, side="left")]
    xs = states[grid]
    return np.einsum("ki,kid->kd", w, xs), np.einsum("ki,kid->kd", w, xs * xs), np.einsum("ki,kid->kd", w, np.abs(xs))


@functools.lru_cache(maxsize=None)
def long_case(model):
    """(problem, x): 201 grid points, dt 0.01, an observation every ten steps from 10 on"""
    return make_problem(model, 3 if model == "L63" else 1, 201, method="euler", dt=0.01, obs_at=list(range(10, 201, 10)))


@functools.lru_cache(maxsize=None)
def long_history(model, n=LONG_N):
    q, x = long_case(model)
    return history_numpy(q, x, None, n, SEED, 0.5)


def fixture_runs():
    """every (case, start, particles, ess_fraction) tests/test_particle_backward_moments.py runs on the fixtures; the seed is SEED"""
    return [(tag, start, n, frac) for tag, start in BCASES for n in SIZES for frac in FRACTIONS]


def lineage_ess(hist):
    t = descendant_weights(hist["lw"], hist["ancestors"], hist["resampled"])
    return 1.0 / np.sum(t * t, axis=1)


# ---- 1, 2: the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d12_euler_p", "quiet_l96d12"])
def test_rows_sum_to_one(tag):
    q, x, _ = case(tag)
    for n in (17, 65):
        for frac in FRACTIONS:
            hist = history(tag, "drawn" if tag in FIXTURES else "given", n, frac)
            table, ess, bmax = backward_weights_numpy(q, x, SEED, hist)
            assert np.all(table >= 0.0) and np.all(np.abs(table.sum(axis=1) - 1.0) <= 4 * n * UNIT), (tag, n, frac)
            assert np.all(ess >= 1.0 - 1e-12) and np.all(ess <= n + 1e-9)
            assert np.array_equal(np.isfinite(bmax), np.asarray(hist["resampled"], dtype=bool))


@pytest.mark.parametrize("tag", ["ou_euler", "l63_euler_p", "l96d12_euler_p"])
def test_without_resampling_it_is_the_genealogy(tag):
    """ess_fraction 0, and one particle: no cut recurses, the table is descendant_weights' bit for bit, and the moments are
    particle_moments_numpy's -- sums of at most 17 products, each rounded once, added in another order: 17 2^-52 of sum W |x| and sum W x^2"""
    q, x, x0 = case(tag)
    for s0 in (None, x0):
        for n, frac in ((17, 0.0), (1, 1.0)):
            hist = history_numpy(q, x, s0, n, SEED, frac)
            table, ess, bmax = backward_weights_numpy(q, x, SEED, hist)
            assert not hist["resampled"].any() and np.all(np.isnan(bmax))
            assert np.array_equal(table, descendant_weights(hist["lw"], hist["ancestors"], hist["resampled"]))
            want = particle_moments_numpy(q, x, s0, n, SEED, frac)
            assert np.array_equal(ess, want["lineage_ess"])
            m1, m2, _ = smoothing_moments(table, replay_numpy(q, x, s0, SEED, hist), hist["obs_t"])
            assert np.all(np.abs(m1 - want["m1"]) <= 17 * 2 * UNIT * want["a1"]) and np.all(np.abs(m2 - want["m2"]) <= 17 * 2 * UNIT * want["m2"])


# ---- 3: where the clouds lie many widths apart -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [t for t in FIXTURES if t.startswith("l96")])
def test_lorenz96_fixtures_return_the_genealogy(tag):
    """the particles of a Lorenz-96 fixture's cloud lie many transition widths apart, so P is the genealogy's indicator up to a leak
    max_s (1 - P_{s, anc[s]}), which the longdouble twin measures.  Where the leak is below 2^-53 -- P is one-hot in fp64: every cut at
    D = 40, most at D = 17 -- every row of the descendant weights is, within the bound, the backward step from the row above it.
    Everywhere, |W^j_i - (descendant weights)_i| = |sum_s W_s (P_{s,i} - 1[i = anc_s])| <= the leak, and one floor.  Measured: at D = 12
    the leak reaches 6.1e-6 (n = 300, the cut at grid index 40), 1.3e-11 (n = 65) and 3.9e-14 (n = 17); at D = 17 9.1e-15 (n = 300); at
    D = 40 it is below 1e-42: D = 12 is not one-hot to rounding, and the rounding bound is not asserted on those cuts."""
    q, x, _ = case(tag)
    worst, leaks, exact = 0.0, [], 0
    for n in (17, 65, 300):
        for frac in FRACTIONS:
            hist = history(tag, "drawn", n, frac)
            assert hist["resampled"].any()
            want = descendant_weights(hist["lw"], hist["ancestors"], hist["resampled"])
            for j in np.flatnonzero(hist["resampled"]):
                e_k, e_o, bmax = step_errors(q, x, SEED, hist, int(j), want[j + 1], want[j])
                leaks.append(bmax.leak)
                got, _ = backward_step(q, x, SEED, hist, int(j), want[j + 1])
                assert np.max(np.abs(got - want[j])) <= bmax.leak + 64 * UNIT, (tag, n, frac, j, bmax.leak)
                if bmax.leak < UNIT:
                    exact += 1
                    worst = max(worst, ratio(e_k, e_o))
                    assert within(e_k, e_o), (tag, n, frac, j, e_k, e_o)
            assert np.allclose(backward_weights_numpy(q, x, SEED, hist)[1], lineage_ess(hist), rtol=1e-4)
    print(tag, f"largest leak {max(leaks):.3g}; {exact} of {len(leaks)} cuts one-hot in fp64, descendant weights against the backward step there: "
          f"worst e_k / max(e_o, 1) = {worst:.3g}")
    assert exact == len(leaks) or tag != "l96d40_rk4_p"
    assert exact > 0 or tag == "l96d12_euler_p"


# ---- 4: Lorenz-96 where the table has something to decide ---------------------------------------------------------------------------------------
MUTANTS = {
    "the drift times 1 + 2^-30": dict(drift=lambda model, theta, z: MUTANT * model_drift(model, theta, z)),
    "1 / R times 1 + 2^-30": dict(divisor=lambda r: r / MUTANT),
    "x~ - z times 1 + 2^-30": dict(target=lambda z, xt: z + MUTANT * (xt - z)),
    "the hlw term left out": dict(hlw=lambda lw: np.zeros_like(lw)),
}


@pytest.mark.parametrize("n", sorted({n for n, _ in TIGHT_RUNS}))
@pytest.mark.parametrize("d", TIGHT)
def test_tight_clouds_react_to_the_kernel(d, n):
    """stretch 0 rests on more than the genealogy's lineages, the float64 restatement holds the bound against its twin with room to spare
    (the floor covers the oracle), and a mutant of the drift, of 1 / R, of the successor or of the hlw term does not"""
    q, x = tight_case(d)
    hist = history_numpy(q, x, None, n, SEED, 1.0)
    assert hist["resampled"][0] == 1
    table, ess, bmax = backward_weights_numpy(q, x, SEED, hist)
    print(f"tight D={d} n={n}: smoothing ESS {ess}, lineage ESS {lineage_ess(hist)}, Bmax {bmax}")
    assert ess[0] > lineage_ess(hist)[0]
    e_k, e_o, _ = step_errors(q, x, SEED, hist, 0, table[1], table[0])
    assert e_k == e_o and e_o <= 1.0, (e_k, e_o)
    for name, hooks in MUTANTS.items():
        got, _ = backward_step(q, x, SEED, hist, 0, table[1], **hooks)
        m_k, m_o, _ = step_errors(q, x, SEED, hist, 0, table[1], got)
        print(f"    {name}: {ratio(m_k, m_o):.3g} times the right-hand side's unit")
        assert not within(m_k, m_o), (name, m_k, m_o)


# ---- 5: many observations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", LONG)
def test_many_observations(model):
    """20 observations, 128 particles: the first stretch of the genealogy rests on one lineage; the backward weights on strictly more (OU,
    double well; Lorenz-63 gains in the middle of the record, not at its start)"""
    q, x = long_case(model)
    hist = long_history(model)
    assert 16 <= int(hist["resampled"].sum()) <= 19 and np.all(np.isfinite(hist["hlw"][np.asarray(hist["resampled"], dtype=bool)]))
    table, ess, _ = backward_weights_numpy(q, x, SEED, hist)
    old = lineage_ess(hist)
    print(f"{model} n={LONG_N}: smoothing ESS stretch 0 / middle {ess[0]:.2f} / {ess[10]:.2f}, lineage ESS {old[0]:.2f} / {old[10]:.2f}")
    assert np.all(np.abs(table.sum(axis=1) - 1.0) <= 1e-12)
    if model != "L63":
        assert ess[0] > old[0]
    assert ess.sum() > old.sum()


# ---- 6: the exact anchor: a linear-Gaussian chain -----------------------------------------------------------------------------------------------
def test_rts_anchor():
    """ou_euler with A_t = theta, 2048 particles, seeds 1 - 8: the seed-mean of the smoothing mean and variance under the backward weights
    within 4 standard errors of the exact marginals at grid index 0, the two observations and grid index 100"""
    q, _, _ = case("ou_euler")
    n_pts = int(q.n_pts)
    assert n_pts == 101 and np.asarray(q.obs_t).size == 2
    x = np.concatenate((np.full(n_pts, float(q.theta)), np.zeros(n_pts)))      # A_t = theta, b_t = 0: the proposal is the model
    ms, ps = rts_marginals(q)
    at = np.array(sorted({0, 100} | {int(t) for t in np.ravel(q.obs_t)}))
    mean, var = [], []
    for seed in range(1, 9):
        hist = history_numpy(q, x, None, 2048, seed, 0.5)
        assert hist["resampled"].sum() >= 1
        table, ess, _ = backward_weights_numpy(q, x, seed, hist)
        m1, m2, _ = smoothing_moments(table, replay_numpy(q, x, None, seed, hist), hist["obs_t"])
        mean.append(m1[at, 0])
        var.append(m2[at, 0] - m1[at, 0] ** 2)
        print(f"seed {seed}: smoothing ESS {ess}, lineage ESS {lineage_ess(hist)}")
    mean, var = np.array(mean), np.array(var)
    se_m, se_v = mean.std(axis=0, ddof=1) / np.sqrt(8.0), var.std(axis=0, ddof=1) / np.sqrt(8.0)
    print("grid indices", at)
    print("exact mean", ms[at], " seed-mean", mean.mean(axis=0), " standard error", se_m)
    print("exact var ", ps[at], " seed-mean", var.mean(axis=0), " standard error", se_v)
    assert np.all(np.abs(mean.mean(axis=0) - ms[at]) <= 4.0 * se_m)
    assert np.all(np.abs(var.mean(axis=0) - ps[at]) <= 4.0 * se_v)


# ---- the conditions of the GPU tests' cases, and the floor ------------------------------------------------------------------------------------
def test_conditions_of_the_gpu_runs():
    """what tests/test_particle_backward_moments.py relies on, on the restatement's histories (the device's decisions are the
    restatement's where the margins of test_particle_filter_cpu hold; the GPU tests compare on the device's own histories and need no
    margin): every fixture case resamples at some size, so that the recursion runs; the quiet case mixes carried and resampled clouds; the
    placement and batch cases resample; the log-weights a resampling replaces are finite"""
    for tag, start in BCASES:
        seen = 0
        for n in (17, 65):
            hist = history(tag, start, n, 1.0)
            flags = np.asarray(hist["resampled"], dtype=bool)
            seen += int(flags.sum())
            assert np.all(np.isfinite(hist["hlw"][flags])), (tag, n)
        assert seen > 0, tag
    quiet = history("quiet_l96d12", "given", 65, 0.5)["resampled"]
    assert 0 < quiet.sum() < quiet.size
    for model, d in (("L63", 3), ("L96", 12)):
        for obs_at in PLACEMENTS:
            q, x = placement_case(model, d, obs_at)
            assert history_numpy(q, x, None, 17, SEED, 1.0)["resampled"].any()
        probs, xs = batch_case(model, d, 20)
        assert any(history_numpy(probs[k], xs[k], None, 40, SEED_BATCH, 0.5, index=k)["resampled"].any() for k in range(3))


def test_floor_is_reported():
    """Bmax and the floor's relative size 2^-53 ((4 + levels(D)) Bmax + 2 + 2 levels(n)), per family of cases (the figures of DESIGN.md
    s.4.24).  The float64 restatement stays within one floor of its twin but for Lorenz-63 with a given start (1.03 floors: every particle
    of the first cloud starts from one state, and x~ - mu is a difference of nearly equal numbers); asserted: within the bound's own factor"""
    rows = []
    for label, q, x, hist in ([(tag, *case(tag)[:2], history(tag, start, 65, 1.0)) for tag, start in BCASES] +
                              [(f"tight D={d}", *tight_case(d), history_numpy(*tight_case(d), None, 65, SEED, 1.0)) for d in TIGHT] +
                              [(f"long {m}", *long_case(m), long_history(m)) for m in LONG]):
        table, _, bmax = backward_weights_numpy(q, x, SEED, hist)
        n, d = table.shape[1], int(q.dim_d)
        top = float(np.nanmax(bmax))
        worst = 0.0
        for j in np.flatnonzero(hist["resampled"])[:2]:
            e_k, e_o, _ = step_errors(q, x, SEED, hist, int(j), table[j + 1], table[j])
            worst = max(worst, e_o)
        rows.append((label, top, UNIT * ((4 + xr.levels(d)) * top + 2 + 2 * xr.levels(n)), worst))
        print(f"{label:>16}: Bmax {top:10.2f}   floor (relative) {rows[-1][2]:.2e}   float64 restatement against its twin: {worst:.3f} floors")
    assert all(np.isfinite(r[1]) and r[3] <= FACTOR for r in rows), rows


# ---- the form of the scores: which one the device may use -------------------------------------------------------------------------------------
def test_gram_form_holds_the_bound():
    """The issue's rule for D >= 5: the cross term goes to the matrix cores -- q = (|a|^2 + |m|^2) - 2 <a, m>, centred on the cloud's mean
    and scaled by 1 / R -- only if that form holds the rounding bound.  Here the form, in float64, against the longdouble twin of the plain
    form, on every resampled cut of every fixture case at n = 65 and 300, the tight cases and the 20-observation cases: it holds
    err_k <= 32 max(err_o, 1) everywhere (worst about 1; at D = 40 and 64 below 1e-4, the tight cases below 0.3), and the cloud's squared
    radius in transition widths, rho^2, which sizes its cancellation, stays below Bmax at D >= 12.  So the device builds it for D >= 5."""
    runs = [(f"{tag} n={n}", *case(tag)[:2], history(tag, start, n, 1.0)) for tag, start in BCASES for n in (65, 300)]
    runs += [(f"tight D={d} n=65", *tight_case(d), history_numpy(*tight_case(d), None, 65, SEED, 1.0)) for d in TIGHT]
    runs += [(f"long {m}", *long_case(m), long_history(m)) for m in LONG]
    worst = 0.0
    for label, q, x, hist in runs:
        table, _, _ = backward_weights_numpy(q, x, SEED, hist)
        top, rho2, bm = 0.0, 0.0, 0.0
        for j in np.flatnonzero(hist["resampled"]):
            got, info = backward_step(q, x, SEED, hist, int(j), table[j + 1], gram=True)
            e_k, e_o, bmax = step_errors(q, x, SEED, hist, int(j), table[j + 1], got)
            top, rho2, bm = max(top, ratio(e_k, e_o)), max(rho2, info.rho2), max(bm, float(bmax))
            assert within(e_k, e_o), (label, int(j), e_k, e_o)
        worst = max(worst, top)
        print(f"{label:>24}: D = {int(q.dim_d):2d}  Gram form e_k / max(e_o, 1) = {top:.3g}   rho^2 {rho2:9.1f}   Bmax {bm:9.1f}")
    print("worst over the cases:", worst)


# ---- 7: the record and the surface -------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    mom = np.arange(4 * 2 * 3, dtype=float).reshape(4, 2, 3) + 1.0
    mom[:, 1] += mom[:, 0] ** 2
    w = np.array([[0.5, 0.5], [0.25, 0.75], [0.25, 0.75], [1.0, 0.0]])
    rec = BackwardSmoothingMoments([-700.0, -701.0], mom, 3, 11, [0, 4, 10], [2.0, 1.6, 1.6, 1.0], w, [2.0, 1.0, 1.5], [1, 0, 1])
    assert len(rec) == 2 and np.array_equal(rec.grid, [0, 3, 6, 9]) and rec.resampled.dtype == bool
    assert np.array_equal(rec.mean, mom[:, 0]) and np.array_equal(rec.var, mom[:, 1] - mom[:, 0] ** 2) and np.allclose(rec.std ** 2, rec.var, rtol=1e-14)
    assert np.array_equal(rec.smoothing_ess_on_grid(), [2.0, 1.6, 1.6, 1.6]) and np.array_equal(rec.weights, w)
    assert abs(rec.log_evidence() - (-700.0 + np.log(1.0 + np.exp(-1.0)) - np.log(2.0))) <= 1e-12
    assert BackwardSmoothingMoments([-700.0], mom[:, :, :1], 3, 11, [0, 4, 10], [1.0] * 4, single_dim=True).mean.shape == (4,)
    for bad in (dict(smoothing_ess=[1.0, 1.0]), dict(weights=w[:3]), dict(moments=mom[:3])):
        args = dict(log_w=[-700.0, -701.0], moments=mom, stride=3, n_pts=11, obs_t=[0, 4, 10], smoothing_ess=[2.0, 1.6, 1.6, 1.0], weights=w)
        args.update(bad)
        with pytest.raises(ValueError):
            BackwardSmoothingMoments(**args)
    assert "genealogy" in BackwardSmoothingMoments.__doc__ and "widths apart" in BackwardSmoothingMoments.__doc__


def test_symbol_and_prototype():
    assert "vgpa_particle_backward_moments" in _lib.SYMBOLS and "vgpa_particle_replaced_logw" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_backward_moments\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    assert " ".join(proto.group(1).split()) == (
        "vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed, double ess_fraction, "
        "const double* prior_mu_or_null, const double* prior_tau_or_null, double* logw, double* state, double* moments, "
        "double* smoothing_ess_or_null, double* weights_or_null, double* ess_or_null, int32_t* resampled_or_null")
    assert re.search(r"int\s+vgpa_particle_replaced_logw\s*\(\s*vgpa_ctx\*\s*ctx,\s*int32_t\s+n_paths,\s*double\*\s*hlw\s*\)\s*;", header)
    with open(os.path.join(ROOT, "vgpa_amd", "build.py")) as fh:
        assert '"particle_smooth.hip"' in fh.read()


def test_python_surface():
    for owner, name, params in [(va.Context, "particle_backward_moments", ["n_paths", "seed", "stride", "ess_fraction", "x", "x0", "prior", "weights"]),
                                (va.VarGP, "backward_moments", ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"]),
                                (va.ProblemBatch, "backward_moments", ["n_paths", "seed", "stride", "ess_fraction", "x", "x0"])]:
        fn = getattr(owner, name, None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, (owner.__name__, list(sig))
        assert sig["stride"].default == 1 and sig["ess_fraction"].default == 0.5 and sig["x"].default is None and sig["x0"].default is None
    assert callable(getattr(va.Context, "particle_replaced_logw", None))
    assert va.BackwardSmoothingMoments is BackwardSmoothingMoments and "BackwardSmoothingMoments" in va.__all__
    assert list(inspect.signature(BackwardSmoothingMoments.__init__).parameters)[1:] == [
        "log_w", "moments", "stride", "n_pts", "obs_t", "smoothing_ess", "weights", "ess", "resampled", "single_dim"]
