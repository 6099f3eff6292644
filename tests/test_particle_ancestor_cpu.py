"""
The cases, conditions, floors and mutants of test_particle_ancestor.py (GPU), asserted without a device on the restatements of
test_particle_gibbs_cpu and test_particle_backward_cpu.  The GPU module imports everything from here and only runs the device and
compares (DESIGN.md s.4.18 "Tests").

A. Decisive cases.  In the fixtures the clouds lie many transition widths apart, so the quadratic form of the pinned slot's ancestor
   score identifies slot 0 whatever the drift is.  decisive_case(model, d) builds, for OU, DW, L63 and L96 at D = 5, 17, 64, a problem in
   which the transition term decides at every cut.  tight_case's idea -- the start's law a few transition widths wide, the prior equal to
   it, wide observation noise (R_obs = 100 I), ess_fraction 1, dt = 0.05 -- with three changes:
     the proposal follows the model: m_k is the solution of the model ODE from the start (`skeleton`), A_t = a I + 0.05 noise and
       b_t = (m_{k+1} - m_k) / dt + A_t m_k, so every particle is pulled to m_k with dt a = 0.4 .. 1 (the cloud stays one to two transition
       widths wide in every component at EVERY cut, not at index 0 alone), the reference -- a trajectory of this proposal -- moves as the
       model moves (x~ lies inside the cloud of transition means), and g - f is small on the cloud (the weights stay comparable);
     the start sits where dt |f| is several R_dd (OU theta = 8 from 3, DW from 2: 6 R; L63 from (-8, -10, 25); L96 on its attractor);
     Sigma is diagonal with entries spanning a factor 8 (L63: 0.5, 1.5, 4; L96: 0.25 .. 2, geometric, the smallest two at d = 0 and D - 1,
       where the circle's two wraps enter).
   41 grid points, 11 observations at CUTS (index 0 and the adjacent pair 0, 1 among them), all resampled; 2, 64, 65, 256, 257 and 300
   particles up to D = 5, 65 and 257 at D = 17 and 64.  Asserted: the construction in numbers; GAP, BOUNDARY and MARGIN for every run, no
   draw excluded; every mutant of MUTANTS, applied to the score at every resampled cut of the unmutated run's own clouds and weights,
   changes a pinned-slot ancestor in every case it applies to (a flip counts where the mutant's winner keeps GAP too); the coverage
   conditions over the whole table of winners (second pass, every wave, odd and even, slot 0); the drift, divisor and successor mutants
   change the backward simulation's table on the same problems (65 particles, 17 trajectories); a batch of three with own theta, Sigma,
   counts and times, where problem 0's theta and R used for all three change a draw of problems 1 and 2.
B. Placement: test_particle_filter_cpu.placement_case (index 0, adjacent indices, the last index) through the conditional filter at 17
   particles; in 5 of the 12 runs the table changes between slot 0 and another slot across an adjacent pair of observations, and there
   the fill that counts t_m <= k for t_m < k breaks an identity.
C. The pinned weight: log_w[0] without resampling is start term + path term + obs term of the reference, a function of inputs the host
   supplied.  pinned_weight evaluates it in longdouble and in float64 (extended_ref.start_term, path_term, obs_term); the floor is the sum
   of the three sizes; conditional_filter_numpy in the device's place stays within one floor (worst 0.31) on B = 3 problems with own
   parameters, given and drawn start, a drawn and a smooth reference (increments of 4.7 R per step), 1 and 65 particles.  The mutant
   dt (1 + 2^-30) inside eta* is the sixth of test_particle_rounding_cpu.test_mutants.

Measured here (every test prints its own figures): flipped draws per mutant and case, of 11 per run --
  mu = x 16 .. 56 of 66 (20, 21 of 22 at D = 17, 64); mu = x - dt f 23 .. 62 (22 of 22); L63 theta_1 <-> theta_2 57, component 1's formula
  for component 2 44; L96 d2 not wrapped 39 / 11 / 9 (D = 5 / 17 / 64), up not wrapped 42 / 12 / 8; DW cubic's sign 39; OU theta from the
  wrong word 19; divisor R_00 30 (L63), 35 / 14 / 14; x~ = ref[k] 12 (DW) .. 55 (20, 19 of 22); the weights after the reset 11 (OU) .. 49 (20 of 22);
  halves of the Philox call swapped 62 / 64 (OU / DW), 41, 21 / 6 / 3; candidates >= 256 ignored 1 .. 2 per case
the smallest gap 1.7e-3, the smallest margin 5.5e-9 S, 308 winners: 8 in the second pass, 147 / 17 / 21 / 44 per wave, 95 odd, 79 slot 0.
"""
import dataclasses
import functools

import numpy as np
import pytest

from test_gpu_edge_cases import make_problem
from test_particle_filter_cpu import BATCH_TIMES, MARGIN, PLACEMENTS, SEED, _given, placement_case
from test_particle_paths_cpu import pick_slots, rewalk_numpy, trace_slots
from test_particle_backward_cpu import GAP as BACKWARD_GAP, backward_slots_numpy, history_numpy
from test_particle_gibbs_cpu import (BOUNDARY, GAP, REF_PARTICLES, REF_SEED, check_identities, conditional_filter_numpy,
                                     conditional_trajectory_numpy, pinned_draw)
from test_particle_rounding_cpu import F64, LD, WORST, _theta, floor_covers_the_oracle, record, xr
from test_path_weights_cpu import _sigma_diag, _split
from test_sample_paths_cpu import model_drift

DT = 0.05
N_PTS = 41
CUTS = (0, 1, 5, 9, 13, 17, 21, 25, 29, 33, 37)      # index 0, the adjacent pair (0, 1), none at the last index: every one can be resampled
DECISIVE = [("OU", 1), ("DW", 1), ("L63", 3), ("L96", 5), ("L96", 17), ("L96", 64)]
BACKWARD_PARTICLES, BACKWARD_DRAWS = 65, 17
# the seed of a run where it is not SEED.  With 257 particles one candidate lies in the second pass of k_pf_cresample, and "candidates >= 256
# ignored" changes a draw only where that one wins: of the seeds 1, 2, ... the first at which it does with every margin kept and every other
# mutant changing two draws of the run or more
CASE_SEED = {("L96", 17, 257): 50, ("L96", 64, 257): 63}


def particles(d):
    """one candidate beside the pinned one, a full wave, one more, one full pass of k_pf_cresample, one more, and two partial passes"""
    return (2, 64, 65, 256, 257, 300) if d <= 5 else (65, 257)


def skeleton(model, theta, start, steps=N_PTS - 1, dt=DT, sub=10):
    """(steps + 1, D): the model ODE's solution from `start` at the grid's times (classical Runge-Kutta, `sub` substeps per grid step)"""
    def f(z):
        return model_drift(model, theta, z[None, :])[0]
    h, out = dt / sub, [np.asarray(start, dtype=float).copy()]
    for _ in range(steps * sub):
        z = out[-1]
        k1 = f(z)
        k2 = f(z + 0.5 * h * k1)
        k3 = f(z + 0.5 * h * k2)
        k4 = f(z + h * k3)
        out.append(z + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4))
    return np.array(out[::sub])


# (model, D) -> (a: A_t = a I + a small perturbation, the start's width in R).  In 64 dimensions a weaker contraction than dt a = 0.7 leaves
# the cloud so wide that every draw returns slot 0, a stronger one spreads the weights further
KNOBS = {("OU", 1): (14.0, 1.4), ("DW", 1): (14.0, 1.4), ("L63", 3): (8.0, 1.4), ("L96", 5): (8.0, 1.4), ("L96", 17): (20.0, 3.0),
         ("L96", 64): (14.0, 1.4)}


@functools.lru_cache(maxsize=None)
def decisive_case(model, d, a=None, width=None, cuts=CUTS, variant=0):
    """(problem, x) -- see the module's docstring.  variant k > 0 (the batch): theta (1 + 0.1 k), Sigma's diagonal rolled by k places and
    times 1 + 0.3 k, other random inputs, the observations at `cuts`"""
    a, width = (KNOBS[model, d][0] if a is None else a), (KNOBS[model, d][1] if width is None else width)
    q, _ = make_problem(model, d, N_PTS, method="euler", dt=DT, obs_at=list(cuts))
    rng = np.random.default_rng(1000 + d + 100 * variant)
    m = len(cuts)
    if model in ("OU", "DW"):
        theta, start, sg = (8.0, 3.0, 0.8) if model == "OU" else (1.0, 2.0, 0.8)      # f(start) = -24 in both: dt |f| = 6 R
        sk = skeleton(model, theta, np.array([start]))[:, 0]
        lin_a = a + 0.05 * rng.standard_normal(N_PTS)
        off_b = np.append(np.diff(sk), sk[-1] - sk[-2]) / DT + lin_a * sk
        s0 = width ** 2 * sg * DT
        q = dataclasses.replace(q, theta=theta, sigma=sg, m0=start, s0=s0, mu0=start, tau0=s0, obs_y=sk[list(cuts)] + rng.standard_normal(m),
                                obs_noise=100.0)
        return q, np.concatenate((lin_a, off_b))
    if model == "L63":
        theta, start, sg = np.array([10.0, 28.0, 2.667]), np.array([-8.0, -10.0, 25.0]), np.array([0.5, 1.5, 4.0])
    else:
        theta, sg = 8.0, rng.permutation(np.geomspace(0.25, 2.0, d))
        start = skeleton(model, theta, 8.0 + rng.standard_normal(d), steps=100)[-1]      # (5 time units: on the attractor)
        # the two wraps of the circle enter f_0 and f_{D-1} alone; 1 / R is the weight they have in the score: the smallest two Sigma_dd there
        for at, rank in ((0, 0), (d - 1, 1)):
            lo = np.argsort(sg)[rank]
            sg[[at, lo]] = sg[[lo, at]]
    theta, sg = theta * (1.0 + 0.1 * variant), np.roll(sg, variant) * (1.0 + 0.3 * variant)
    sk = skeleton(model, theta, start)
    lin_a = a * np.eye(d) + 0.05 * rng.standard_normal((N_PTS, d, d))
    off_b = np.concatenate((np.diff(sk, axis=0), sk[-1:] - sk[-2:-1])) / DT + np.einsum("kij,kj->ki", lin_a, sk)
    s0 = np.diag(width ** 2 * sg * DT)
    q = dataclasses.replace(q, theta=theta, sigma=np.diag(sg), m0=sk[0].copy(), s0=s0, mu0=sk[0].copy(), tau0=s0.copy(),
                            obs_y=sk[list(cuts)] + rng.standard_normal((m, d)), obs_noise=100.0 * np.eye(d))
    return q, np.concatenate((lin_a.ravel(), off_b.ravel()))


def case_seed(model, d, n):
    return CASE_SEED.get((model, d, n), SEED)


def drawn_reference(q, x, x0=None, index=0, seed=REF_SEED, ess_fraction=1.0):
    """one trajectory of the particle_paths restatement at another seed (read-only): the reference of a conditional run"""
    hist = history_numpy(q, x, x0, REF_PARTICLES, seed, ess_fraction, index=index)
    final, _ = pick_slots(hist["lw"], 1, seed, int(q.n_pts), index=index)
    path = rewalk_numpy(q, x, x0, seed, trace_slots(final, hist["ancestors"], hist["resampled"]), index=index)[0]
    path.setflags(write=False)
    return path


@functools.lru_cache(maxsize=None)
def decisive_reference_path(model, d):
    return drawn_reference(*decisive_case(model, d))


@functools.lru_cache(maxsize=None)
def decisive_reference(model, d, n):
    """(history, trajectory, table, pick margin) of a decisive run, computed once per process (read-only)"""
    q, x = decisive_case(model, d)
    ref, seed = decisive_reference_path(model, d), case_seed(model, d, n)
    hist = conditional_filter_numpy(q, x, None, ref, n, seed, 1.0)
    return (hist,) + conditional_trajectory_numpy(q, x, None, ref, seed, hist)


@functools.lru_cache(maxsize=None)
def decisive_backward(model, d):
    """(history, final slots, table, gaps) of the backward simulation on a decisive case: BACKWARD_PARTICLES particles, BACKWARD_DRAWS
    trajectories, SEED, ess_fraction 1"""
    q, x = decisive_case(model, d)
    hist = history_numpy(q, x, None, BACKWARD_PARTICLES, SEED, 1.0)
    final, _ = pick_slots(hist["lw"], BACKWARD_DRAWS, SEED, int(q.n_pts))
    table, gaps = backward_slots_numpy(q, x, SEED, hist, final)
    return hist, final, table, gaps


def decisive_runs():
    return [(model, d, n) for model, d in DECISIVE for n in particles(d)]


# ---- the mutants -----------------------------------------------------------------------------------------------------------------------------
def _l63(change):
    def drift(model, theta, z):
        return change(np.asarray(theta, dtype=float), z)
    return drift


def _l63_swapped(theta, z):
    return model_drift("L63", theta[[0, 2, 1]], z)


def _l63_component(theta, z):
    f = model_drift("L63", theta, z)
    f[:, 2] = f[:, 1]
    return f


def _l96_d2(model, theta, z):
    """d2 = d - 2 not wrapped at d = 0: the index clamped to 0 in D - 2's place"""
    d2 = np.roll(z, 2, axis=1)
    d2[:, 0] = z[:, 0]
    return (np.roll(z, -1, axis=1) - d2) * np.roll(z, 1, axis=1) - z + theta


def _l96_up(model, theta, z):
    """up = d + 1 not wrapped at d = D - 1: the index clamped to D - 1 in 0's place"""
    up = np.roll(z, -1, axis=1)
    up[:, -1] = z[:, -1]
    return (up - np.roll(z, 2, axis=1)) * np.roll(z, 1, axis=1) - z + theta


# name -> (the models it applies to, the smallest particle count it applies to, pinned_draw's hooks, backward_slots_numpy's hooks or None)
MUTANTS = {
    "mu = x": (None, 2, dict(drift=lambda model, theta, z: np.zeros_like(z)), dict(drift=lambda model, theta, z: np.zeros_like(z))),
    "mu = x - dt f": (None, 2, dict(drift=lambda model, theta, z: -model_drift(model, theta, z)),
                      dict(drift=lambda model, theta, z: -model_drift(model, theta, z))),
    "L63: theta_1 <-> theta_2": (("L63",), 2, dict(drift=_l63(_l63_swapped)), dict(drift=_l63(_l63_swapped))),
    "L63: component 1's formula for component 2": (("L63",), 2, dict(drift=_l63(_l63_component)), dict(drift=_l63(_l63_component))),
    "L96: d2 not wrapped at d = 0": (("L96",), 2, dict(drift=_l96_d2), dict(drift=_l96_d2)),
    "L96: up not wrapped at d = D - 1": (("L96",), 2, dict(drift=_l96_up), dict(drift=_l96_up)),
    "DW: the cubic's sign": (("DW",), 2, dict(drift=lambda model, theta, z: 4.0 * z * (theta + z * z)),
                             dict(drift=lambda model, theta, z: 4.0 * z * (theta + z * z))),
    # (the words behind a one-parameter model's theta are the padding of the parameter array: 0)
    "OU: theta from the wrong word": (("OU",), 2, dict(drift=lambda model, theta, z: -0.0 * z), dict(drift=lambda model, theta, z: -0.0 * z)),
    "divisor R_00 for every d": (("L63", "L96"), 2, dict(divisor=lambda r: np.full_like(r, r[0])), dict(divisor=lambda r: np.full_like(r, r[0]))),
    "x~ = ref[k]": (None, 2, dict(target=lambda ref, k: ref[k]), dict(target=lambda z, xt: z)),
    "the weights after the reset": (None, 2, dict(weights=np.zeros_like), None),
    "odd and even halves of the Philox call swapped": (None, 2, dict(swap_halves=True), None),
    "candidates >= 256 ignored": (None, 257, dict(limit=256), None),
}
BACKWARD_MUTANTS = [name for name, spec in MUTANTS.items() if spec[3] is not None]      # the drift mutants, the divisor and the successor


def applies(name, model, n=None):
    models, least = MUTANTS[name][:2]
    return (models is None or model in models) and (n is None or n >= least)


def redraw(q, hist, ref, seed, index=0, params=None, **hooks):
    """(winners, gaps): the pinned slot's ancestor at every resampled cut of a run, drawn again from the run's own clouds and weights under
    `hooks`; params: the problem whose theta and R are used (another one's: the batch's mutant)"""
    src = q if params is None else params
    theta = np.asarray(src.theta, dtype=float)
    rdiag = np.linalg.cholesky(_sigma_diag(src) * float(q.dt)).diagonal()
    cuts = np.flatnonzero(hist["resampled"])
    draws = [pinned_draw(q, theta, rdiag, hist["clouds"][j], hist["hlw"][j], ref, int(hist["obs_t"][j]), seed, index, **hooks) for j in cuts]
    return np.array([w for w, _ in draws], dtype=np.int64), np.array([g for _, g in draws])


def flipped(q, hist, ref, seed, hooks, index=0, params=None):
    """the draws of a run a mutant changes -- counted where the mutant's own winner keeps GAP too: a device with that error would return it"""
    got, gaps = redraw(q, hist, ref, seed, index, params, **hooks)
    return int(np.sum((got != pinned_ancestors(hist)) & (gaps >= GAP)))


def pinned_ancestors(hist):
    return hist["ancestors"][np.flatnonzero(hist["resampled"]), 0]


# ---- A: the construction -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", DECISIVE)
def test_the_construction(model, d):
    """what the module's docstring says of a decisive case, in numbers"""
    q, x = decisive_case(model, d)
    sg = _sigma_diag(q).diagonal()
    rdiag = np.sqrt(sg * DT)
    obs_t = np.asarray(q.obs_t).ravel()
    assert int(q.n_pts) == N_PTS and obs_t.size >= 8 and obs_t[0] == 0 and np.any(np.diff(obs_t) == 1) and obs_t[-1] < N_PTS - 1
    if d > 1:
        assert sg.max() / sg.min() >= 8.0 and np.count_nonzero(_sigma_diag(q) - np.diag(sg)) == 0
    f = model_drift(q.model, np.asarray(q.theta, dtype=float), np.reshape(np.asarray(q.m0, dtype=float), (1, d)))[0]
    share = DT * np.abs(f) / rdiag
    rms = float(np.sqrt(np.mean(share * share)))
    print(f"{model} D={d}: dt |f(m0)| / R_dd: root mean square {rms:.2f}, largest {share.max():.2f}")
    assert rms >= 3.0      # (the drift's share of the transition mean, in transition widths, over the components)
    assert np.array_equal(np.asarray(q.mu0, dtype=float).ravel(), np.asarray(q.m0, dtype=float).ravel())
    assert np.array_equal(np.asarray(q.tau0, dtype=float).ravel(), np.asarray(q.s0, dtype=float).ravel())
    for n in particles(d):
        hist = decisive_reference(model, d, n)[0]
        assert int(hist["resampled"].sum()) == obs_t.size >= 8, (n, hist["resampled"])      # every cut is resampled
        assert np.array_equal(redraw(q, hist, decisive_reference_path(model, d), case_seed(model, d, n))[0], pinned_ancestors(hist))


# ---- A: the margins --------------------------------------------------------------------------------------------------------------------------
def test_margins():
    """conditions on the cases, not measurements of the device: every run keeps GAP, BOUNDARY and MARGIN, no draw excluded; the backward
    simulations keep test_particle_backward_cpu's GAP and the filter's MARGIN"""
    for model, d, n in decisive_runs():
        hist, _, _, pick = decisive_reference(model, d, n)
        gap, margin = min(hist["gaps"]), min(hist["margins"])
        print(f"{model} D={d} n={n}: resampled cuts {int(hist['resampled'].sum())}, smallest gap {gap:.3g}, smallest margin {margin:.3g}, pick {pick:.3g}")
        assert gap >= GAP and margin >= BOUNDARY and pick >= MARGIN, (model, d, n)
    for model, d in DECISIVE:
        hist, final, table, gaps = decisive_backward(model, d)
        gap = min(float(g.min()) for g in gaps)
        pick = pick_slots(hist["lw"], BACKWARD_DRAWS, SEED, N_PTS)[1]
        print(f"{model} D={d} backward: draws {len(gaps)} x {BACKWARD_DRAWS}, smallest gap {gap:.3g}, smallest margin {min(hist['margins']):.3g}, pick {pick:.3g}")
        assert gap >= BACKWARD_GAP and min(hist["margins"]) >= MARGIN and pick >= MARGIN, (model, d)
        assert np.all(np.abs(hist["ess"] - BACKWARD_PARTICLES) >= 1e-6)


# ---- A: the mutant table -----------------------------------------------------------------------------------------------------------------
def test_mutant_table():
    """every mutant flips at least one pinned-slot ancestor in every case it applies to (a case: a model and a D, its runs at all particle
    counts together; the count per run is printed)"""
    for name in MUTANTS:
        for model, d in DECISIVE:
            if not applies(name, model):
                continue
            q, _ = decisive_case(model, d)
            ref = decisive_reference_path(model, d)
            flips = {}
            for n in particles(d):
                if applies(name, model, n):
                    hist = decisive_reference(model, d, n)[0]
                    flips[n] = flipped(q, hist, ref, case_seed(model, d, n), MUTANTS[name][2])
            print(f"mutant [{name}] {model} D={d}: flipped draws of {len(CUTS)} per particle count {flips}")
            assert sum(flips.values()) >= 1, (name, model, d)


@pytest.mark.parametrize("model,d", DECISIVE)
def test_backward_mutants(model, d):
    """the drift mutants, the divisor and the successor, applied to the backward restatement, change its table: both statements of mu are
    held to the one numpy model_drift on all four models"""
    q, x = decisive_case(model, d)
    hist, final, table, _ = decisive_backward(model, d)
    assert not np.array_equal(table, trace_slots(final, hist["ancestors"], hist["resampled"]))
    for name in BACKWARD_MUTANTS:
        if applies(name, model):
            other = backward_slots_numpy(q, x, SEED, hist, final, **MUTANTS[name][3])[0]
            flips = int(np.sum(other != table))
            print(f"backward mutant [{name}] {model} D={d}: {flips} of {table[:-1].size} entries")
            assert flips >= 1, name


# ---- A: the coverage conditions --------------------------------------------------------------------------------------------------------------
def test_coverage_conditions():
    """over the whole table of pinned-slot ancestors: a winner in the second pass, in each of the four waves, odd and even, and slot 0"""
    winners = np.concatenate([pinned_ancestors(decisive_reference(*run)[0]) for run in decisive_runs()])
    quarters = np.bincount((winners[winners != 0] % 256) >> 6, minlength=4)
    odd, even = int(np.sum(winners % 2 == 1)), int(np.sum((winners % 2 == 0) & (winners != 0)))
    print(f"winners {winners.size}: second pass {int(np.sum(winners >= 256))}, per wave {quarters.tolist()}, odd {odd}, even (not 0) {even}, "
          f"slot 0 {int(np.sum(winners == 0))}")
    assert np.any(winners >= 256) and np.all(quarters >= 1) and odd >= 1 and even >= 1 and np.any(winners == 0)
    for model, d in DECISIVE:
        mine = np.concatenate([pinned_ancestors(decisive_reference(model, d, n)[0]) for n in particles(d)])
        assert np.any(mine != 0), (model, d)


# ---- A: the batch ----------------------------------------------------------------------------------------------------------------------------
BATCH_MODELS = [("L63", 3), ("L96", 5)]
BATCH_CUTS = [CUTS, (2, 3, 8, 14, 20, 26, 32, 38), (0, 4, 5, 11, 18, 25, 31, 36, 39)]      # own counts and times; an adjacent pair in each
BATCH_PARTICLES = 65


@functools.lru_cache(maxsize=None)
def batch_decisive(model, d):
    """(problems, xs): three decisive problems with their own theta, anisotropic Sigma, observation count and times (theta_v, R_stride and
    n_obs_v of k_pf_cresample's arguments)"""
    cases = [decisive_case(model, d, None, None, BATCH_CUTS[k], k) for k in range(3)]
    return [dataclasses.replace(q, obs_h=np.eye(d)) for q, _ in cases], np.stack([x for _, x in cases])


@functools.lru_cache(maxsize=None)
def batch_decisive_reference(model, d):
    """per problem k: (reference trajectory, history, trajectory, table, pick margin) of the run with BATCH_PARTICLES particles, SEED,
    ess_fraction 1 and counter word k"""
    probs, xs = batch_decisive(model, d)
    out = []
    for k, q in enumerate(probs):
        ref = drawn_reference(q, xs[k], index=k)
        hist = conditional_filter_numpy(q, xs[k], None, ref, BATCH_PARTICLES, SEED, 1.0, index=k)
        out.append((ref, hist) + conditional_trajectory_numpy(q, xs[k], None, ref, SEED, hist, index=k))
    return out


@pytest.mark.parametrize("model,d", BATCH_MODELS)
def test_batch(model, d):
    """the margins of the batch's runs, and one more mutant: problem 0's theta and R used for all three changes a draw of problem 1 and one of
    problem 2; the other mutants, counted over the three problems together"""
    probs, _ = batch_decisive(model, d)
    total = {}
    assert len({tuple(np.atleast_1d(q.theta)) for q in probs}) == 3 and len({np.asarray(q.obs_t).size for q in probs}) == 3
    for k, (ref, hist, _, _, pick) in enumerate(batch_decisive_reference(model, d)):
        q = probs[k]
        sg = _sigma_diag(q).diagonal()
        assert sg.max() / sg.min() >= 8.0 and int(hist["resampled"].sum()) == len(BATCH_CUTS[k]) >= 8
        gap, margin = min(hist["gaps"]), min(hist["margins"])
        print(f"{model} D={d} batch problem {k}: resampled cuts {int(hist['resampled'].sum())}, smallest gap {gap:.3g}, smallest margin {margin:.3g}, pick {pick:.3g}")
        assert gap >= GAP and margin >= BOUNDARY and pick >= MARGIN
        assert np.array_equal(redraw(q, hist, ref, SEED, index=k)[0], pinned_ancestors(hist))
        flips = {name: flipped(q, hist, ref, SEED, MUTANTS[name][2], index=k) for name in MUTANTS if applies(name, model, BATCH_PARTICLES)}
        for name, count in flips.items():
            total[name] = total.get(name, 0) + count
        if k:
            flips["problem 0's theta and R"] = flipped(q, hist, ref, SEED, {}, index=k, params=probs[0])
            assert flips["problem 0's theta and R"] >= 1, (k, flips)
        print(f"{model} D={d} batch problem {k}: flipped draws of {len(BATCH_CUTS[k])} per mutant {flips}")
    assert min(total.values()) >= 1, total


# ---- B: observation placement --------------------------------------------------------------------------------------------------------------
PLACED = [("L63", 3), ("L96", 12)]
PLACED_PARTICLES = 17


def placement_runs():
    return [(model, d, obs_at, start) for model, d in PLACED for obs_at in PLACEMENTS for start in ("drawn", "given")]


@functools.lru_cache(maxsize=None)
def placement_reference(model, d, obs_at, start):
    """(x0 or None, reference trajectory, history, trajectory, table, pick margin): placement_case through the conditional filter with
    PLACED_PARTICLES particles, SEED and ess_fraction 1; the reference drawn as test_particle_gibbs_cpu.batch_reference draws its own"""
    q, x = placement_case(model, d, obs_at)
    x0 = _given(q) if start == "given" else None
    ref = drawn_reference(q, x, x0, ess_fraction=0.5)
    hist = conditional_filter_numpy(q, x, x0, ref, PLACED_PARTICLES, SEED, 1.0)
    return (x0, ref, hist) + conditional_trajectory_numpy(q, x, x0, ref, SEED, hist)


def test_placement():
    """grid index 0, adjacent indices, the last index (whose cloud is never resampled): the margins, the identities, a table that changes
    between slot 0 and another slot across an adjacent pair of observations -- and there the fill that counts t_m <= k breaks an identity"""
    crossing = 0
    for model, d, obs_at, start in placement_runs():
        q, x = placement_case(model, d, obs_at)
        x0, ref, hist, path, table, pick = placement_reference(model, d, obs_at, start)
        gap, margin = min(hist["gaps"], default=np.inf), min(hist["margins"], default=np.inf)
        print(f"{model} D={d} at {obs_at} {start}: resampled {hist['resampled'].tolist()}, table {table.tolist()}, smallest gap {gap:.3g}, margin {margin:.3g}, pick {pick:.3g}")
        assert gap >= GAP and margin >= BOUNDARY and pick >= MARGIN
        # (the decision ESS < n: away from n, or n exactly -- a given start under an observation at index 0, every weight the same)
        assert np.all((np.abs(hist["ess"] - PLACED_PARTICLES) >= 1e-6) | (hist["hlw"].max(axis=1) == hist["hlw"].min(axis=1)))
        if obs_at[-1] == int(q.n_pts) - 1:
            assert hist["resampled"][-1] == 0 and table[-1] == table[-2]
        check_identities(q, hist, path, table, ref)
        obs_t = hist["obs_t"]
        pairs = [j for j in range(obs_t.size - 1) if obs_t[j + 1] == obs_t[j] + 1 and (table[j + 1] == 0) != (table[j + 2] == 0)]
        if pairs:      # (the stretch between the two observations is one grid point long, and the reference's on one side of it alone)
            crossing += 1
            mutant = conditional_trajectory_numpy(q, x, x0, ref, SEED, hist, side="right")[0]
            with pytest.raises(AssertionError):
                check_identities(q, hist, mutant, table, ref)
    print("runs whose table changes between slot 0 and another slot across an adjacent pair:", crossing)
    assert crossing >= 1


# ---- C: the pinned weight to the project's bound ---------------------------------------------------------------------------------------------
WEIGHT_MODELS = [("OU", 1), ("DW", 1), ("L63", 3), ("L96", 5), ("L96", 12), ("L96", 40), ("L96", 64)]
WEIGHT_PARTICLES = (1, 65)
WEIGHT_SEED = 77
WEIGHT_REFERENCES = ("drawn", "smooth")


@functools.lru_cache(maxsize=None)
def weight_case(model, d):
    """(problems, xs): B = 3 with their own theta, Sigma, A_t, b_t, start moments, observation counts and times (index 0, adjacent indices
    and the last index among them), a prior other than the start's law; dt = 0.01"""
    probs, xs = [], []
    for k in range(3):
        q, x = make_problem(model, d, N_PTS, method="euler", seed=40 + k, obs_at=list(BATCH_TIMES[k]))
        if model == "L63":
            x = np.concatenate((x[:N_PTS * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(N_PTS, axis=0).ravel()))
        theta = np.asarray(q.theta, dtype=float) * (1.0 + 0.05 * k)
        q = dataclasses.replace(q, theta=theta if theta.ndim else float(theta), sigma=np.asarray(q.sigma) * (1.0 + 0.1 * k),
                                s0=np.asarray(q.s0) * (1.0 + 0.1 * k), obs_h=None if d == 1 else np.eye(d))
        probs.append(q)
        xs.append(x)
    return probs, np.stack(xs)


@functools.lru_cache(maxsize=None)
def weight_references(model, d, start, kind):
    """(3, Np, D), read-only.  "drawn": per problem one trajectory of the particle_paths restatement; "smooth": a host-made one,
    m0_i + 30 R_ii sin(2 pi k / 40 + i), whose increments (about 4.7 R per step) no noise draw produces: the implied increment eta* is large
    and (ref_k - ref_{k-1}) - dt g cancels for real"""
    probs, xs = weight_case(model, d)
    out = []
    for k, q in enumerate(probs):
        if kind == "drawn":
            out.append(drawn_reference(q, xs[k], _given(q) if start == "given" else None, index=k, ess_fraction=0.5))
        else:
            amp = 30.0 * np.sqrt(_sigma_diag(q).diagonal() * float(q.dt))
            grid = np.arange(N_PTS)[:, None]
            out.append(np.reshape(np.asarray(q.m0, dtype=float), (1, d)) + amp[None, :] * np.sin(2.0 * np.pi * grid / (N_PTS - 1) + np.arange(d)[None, :]))
    out = np.stack(out)
    out.setflags(write=False)
    return out


def pinned_weight(q, x, start, ref, T):
    """(start term + path term + obs term of the reference, the sum of their sizes): what slot 0's log-weight is without resampling"""
    d, n_pts = int(q.dim_d), int(q.n_pts)
    lin_a, off_b = _split(q, x)
    stored = np.reshape(np.asarray(ref, dtype=float), (1, n_pts, d))
    pt, scale, rec = xr.path_term(q.model, _theta(q), _sigma_diag(q).diagonal(), float(q.dt), lin_a.reshape(n_pts, d, d), off_b.reshape(n_pts, d), stored, T=T)
    ot, size = xr.obs_term(q.obs_t, q.obs_y, q.obs_noise, getattr(q, "obs_h", None), stored, T=T)
    value, total = pt[0] + ot[0], scale[0] + rec[0] + size[0]
    if start == "drawn":
        st, ssize = xr.start_term(stored[0, 0], q.mu0, np.reshape(np.asarray(q.tau0, dtype=float), (d, d)), q.m0,
                                  np.reshape(np.asarray(q.s0, dtype=float), (d, d)), T)
        value, total = st + value, total + ssize
    return value, total


def check_pinned_weight(worst, label, family, q, x, start, ref, got):
    ext, size = pinned_weight(q, x, start, ref, LD)
    orc, _ = pinned_weight(q, x, start, ref, F64)
    return record(worst, family, "pinned log_w", label, got, ext, orc, size)


@pytest.mark.parametrize("model,d", WEIGHT_MODELS)
def test_pinned_weight_floor_covers_the_oracle(model, d):
    """conditional_filter_numpy(ess_fraction=0) in the device's place: err <= floor for every problem, start, reference and particle count"""
    probs, xs = weight_case(model, d)
    assert [list(np.asarray(q.obs_t)) for q in probs] == [list(t) for t in BATCH_TIMES]
    for start in ("given", "drawn"):
        for kind in WEIGHT_REFERENCES:
            refs = weight_references(model, d, start, kind)
            for n in WEIGHT_PARTICLES:
                for k, q in enumerate(probs):
                    x0 = _given(q) if start == "given" else None
                    run = conditional_filter_numpy(q, xs[k], x0, refs[k], n, WEIGHT_SEED, 0.0, index=k)
                    assert not run["resampled"].any() and np.array_equal(run["state"][0], refs[k][-1])
                    with floor_covers_the_oracle():
                        assert not check_pinned_weight(WORST, f"{model}{d} {start} {kind} n={n} p={k}", "cpu pinned weight", q, xs[k], start, refs[k],
                                                       run["lw"][0])


def test_print_worst_pinned_weight():
    """(last: the worst err / floor of part C in this run, numpy in the device's place; it must be <= 1)"""
    r = WORST.get(("cpu pinned weight", "pinned log_w"))
    print("WORST cpu pinned weight / pinned log_w:", r)
    assert r is None or r <= 1.0
