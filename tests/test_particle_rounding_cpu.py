"""
The case tables, inputs, floors, regime conditions and mutants of test_particle_rounding.py (GPU), asserted without a device: numpy's
own recursions (sample_paths_numpy, path_weights_numpy, particle_statistics_numpy, particle_paths_numpy, forecast_numpy) stand in for
the kernels of vgpa_amd/csrc/sample.hip.  The GPU module imports everything from here and only runs the device and compares.

The principle.  The older particle tests compare whole paths against a recursion that draws its own normals; the device's log / sincos
differ from numpy's by ulps and Lorenz-63 / Lorenz-96 amplify that along the path, so they cannot go much below 1e-9.  Here EVERY
COMPARISON STARTS FROM DATA THE DEVICE ITSELF RETURNED, OR DATA THE HOST SUPPLIED, AND SPANS AT MOST ONE STEP OF THE RECURSION OR ONE
REDUCTION: chaos never enters, every output is a deterministic function of known fp64 inputs, and it is held to the project's bound

    err_k(q) <= FACTOR * max(err_o(q), floor(q))                                               FACTOR = 32

err_k: what is tested (a kernel; here numpy's recursion, or a mutant of it) against the longdouble restatement of the one step or the
one reduction (tests/extended_ref.py); err_o: the same restatement run in float64 on the same inputs.  Both are reported in units of the
floor, the differences taken in longdouble: `errors` returns max over the entries of |difference| / (2^-53 size), so the bound reads
e_k <= 32 max(e_o, 1), and "the floor covers the oracle" reads e <= 1 (floor_covers_the_oracle: asserted for every comparison with numpy
in the device's place).

The floors (2^-53 times the size; the sizes are computed by the restatements themselves, whose docstrings count the roundings).  With the
sizes as first stated -- the terms of the result alone -- numpy's own evaluation did NOT stay within them: 1.8 floors for a step, 2.4 (and
242 .. 389 under R of cond 1e4) for the obs term, 3.6 .. 7.3 for H, 4 .. 5 for the weighted sums even when added pairwise (28 when added
one term at a time: one dominant weight absorbs 512 small ones), 1.2 for lineage_ess.  What was missing is derivable and is now part of the
floors: every rounding of a careful evaluation counted once, and sums of n terms taken as balanced trees, levels(n) = ceil(log2 n)
additions per term (the restatements add that way: extended_ref._sum).
  a normal xi              (1 + 4 pi) rho, rho = sqrt(-2 ln u1): the angle carries the rounding of the fp64 constant 2 pi and of its product
                           with u2 (each up to 2 pi 2^-53 in the angle, i.e. 2 pi rho 2^-53 in xi), the product rho cos one more
  one step, component i    2 |x_{k-1,i}| + (4 + L) dt a_i + (2 + L) n_i + sum_j |R_ij| (1 + 4 pi) rho_j with a_i = sum_j |A_ij x_j| + |b_i| (model
                           kind: the sum of the drift's |monomials|), n_i = sum_j |R_ij xi_j|, L = levels(D + 1): the two sums of the update, the
                           product dt f, the drift's terms and their tree, the noise's products and their tree (extended_ref.em_step); the
                           last term because the step takes the xi the device computed and the restatement the longdouble xi of the same
                           uniforms, which differ by up to the normal's own floor (without it numpy's own step stood at 10 .. 21 of the
                           first floors where x is small against the noise: OU, D = 2)
  path term of a path      sum_k sum_i |d_i| / Sigma_ii (|x_k,i| + |x_{k-1},i| + dt |g_i|) + sum_k |increment_k|: eta_k is known from the stored
                           states only up to the two roundings of the state update (as stated; numpy stands at 0.16)
  obs term of a path       (5 + 2 levels(D) + levels(M) + cond_2(R)) sum_n q_n + 4 |constant|, q_n = sum_ij |r_i Q_ij r_j| / 2 (extended_ref.obs_term)
  Q_j, G_j of a lineage    sum_k 2 |r_j| (|x_k,j| + |x_{k-1},j| + dt |f_j|) / dt + (1 + levels(Np - 1)) sum_k |summand| (G: |phi_j| in 2 |r_j| / dt's
                           place); H_j: (1 + levels(Np - 1)) sum_k |summand|, and from D = 5 on the constant dt (Np - 1), compared exactly
  sum W v                  sum_i W_i (1 + |lw_i - max lw| + 2 levels(n)) |v_i|: the normalising sum and the sum itself
  lineage_ess              (1 + max |lw - max lw| + 2 levels(n)) times the value

What this module asserts for every case: nothing is excluded (every stored step, every returned entry); the regime conditions (stiff:
0.4 <= dt rho(A_t) <= 1; everything finite; the spread-700 weights not all underflowed); for the resampling runs, a resampling and two
distinct lineages at stretch 0 (their margins are cleared by test_particle_filter_cpu.test_margin_condition: same tags, n, fraction and
seed); and that the floors cover the oracle: err <= floor for every comparison.

Measured here, on the CPU, numpy standing in for the device (worst err in floors; every test prints its own):
  normals 0.47; steps: posterior 0.65, model 0.67, lineage 0.76, backward 0.75, forecast 0.75; path term 0.16, obs term 0.46 (dense R of cond
  1e4: 0.01); rows Q 0.27, G 0.19, H 0.91, their mean 0.36; forecast moments 0.83 / 0.97; smoothing sums 0.52 / 0.95, lineage_ess 0.26
The mutants (test_mutants prints each with its figure on the older check's measure and its factor over the right-hand side of the new bound):
  dt (1 + 2^-30) in the quadratic term of the path increment    older 9.6e-10 (passes) .. 1.03e-9 (at its tolerance), over by 1.7e3 .. 6.2e3
  the drift of one step times 1 + 2^-30                         older 1.7e-11 .. 6.3e-10 (passes), over by 2.0e3 .. 1.5e4
  r^2 (1 / dt) with 1 / dt off by 2^-30 in Q                    older 9.3e-10 (passes), over by 4.3e3 .. 1.5e4
  weights normalised by S (1 + 2^-30)                           older 9.3e-10 (passes), over by 1.2e4 .. 1.6e4
  xi with the fp32 value of 2 pi                                older 8.2e-9 (rejected there too, as by the generator check at 1e-12), over by 3.6e6
  dt (1 + 2^-30) inside eta* of the conditional filter's pinned slot   older 2.5e-11 .. 8.8e-11 (passes; 2.7e-9 on a smooth reference at D = 40),
                                                                over by 2.0e2 .. 3.0e3 (the bound of test_particle_ancestor.py on log_w[:, 0])
"""
import collections
import contextlib
import functools
import types

import numpy as np
import pytest

import extended_ref as xr
from conftest import rel_err
from test_gpu_edge_cases import make_problem, spd
from test_particle_filter_cpu import SEED as PF_SEED, case
from test_particle_forecast_cpu import forecast_numpy
from test_particle_paths_cpu import reference as paths_reference
from test_particle_statistics_cpu import particle_statistics_numpy
from test_path_weights_cpu import TAGS, _sigma_diag, _split, path_weights_numpy
from test_sample_paths_cpu import sample_paths_numpy
from test_stepper_rounding_cpu import stiff_ab

LD = np.longdouble
F64 = np.float64
FACTOR = 32
UNIT = 2.0 ** -53
DT = 0.01
B = 3                        # problems per walk context, each with its own theta, Sigma and A_t
N_PATHS = 65                 # a full block of 64 paths and one more
SEED = 0x1234567890ABCDEF
XI_SIZE = 1.0 + 4.0 * np.pi      # a normal's floor in units of 2^-53 rho
WORST = {}                   # (family, quantity) -> the worst ratio e_k / max(e_o, 1) of this process's CPU run


# ---- the measure ---------------------------------------------------------------------------------------------------------------------------
def errors(got, ext, orc, size):
    """(e_k, e_o): max over the entries of |got - ext| and |orc - ext| in units of 2^-53 size, taken in longdouble.  An entry of size 0 must be
    exact (else inf); a NaN stays a NaN."""
    ext, size = np.asarray(ext, dtype=LD), np.asarray(size, dtype=LD)

    def worst(v):
        diff = np.abs(np.asarray(v, dtype=LD).reshape(ext.shape) - ext)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(diff == 0, LD(0), diff / (UNIT * size))
        return float(np.max(e))

    return worst(got), worst(orc)


def ratio(e_k, e_o):
    return e_k / max(e_o, 1.0)


def within(e_k, e_o):
    return bool(e_k <= FACTOR * max(e_o, 1.0))


_WATCHERS = []               # the lists of floor_covers_the_oracle blocks that are open: record() appends (label, quantity, e_k) to each


@contextlib.contextmanager
def floor_covers_the_oracle():
    """The CPU condition of every floor: numpy stands in for the device inside the block, and every comparison recorded there must satisfy
    err <= floor, that is e_k <= 1 (asserted when the block ends)."""
    seen = []
    _WATCHERS.append(seen)
    try:
        yield seen
    finally:
        _WATCHERS.remove(seen)
    over = [entry for entry in seen if not entry[2] <= 1.0]
    assert seen and not over, over


def record(worst, family, quantity, label, got, ext, orc, size):
    """prints e_o, e_k and their ratio, keeps the worst ratio of (family, quantity), returns the failures (a list: empty, or one entry)"""
    e_k, e_o = errors(got, ext, orc, size)
    for seen in _WATCHERS:
        seen.append((label, quantity, e_k))
    r = ratio(e_k, e_o)
    key = (family, quantity)
    worst[key] = float(np.maximum(worst.get(key, 0.0), r))
    print(f"{label} [{family}] {quantity}: err_o={e_o:.3f} err_k={e_k:.3f} ratio={r:.2f} (units of the floor; {np.size(ext)} entries)")
    return [] if within(e_k, e_o) else [(label, family, quantity, e_o, e_k)]


# ---- A, B: the walk problems -----------------------------------------------------------------------------------------------------------------
Walk = collections.namedtuple("Walk", "kind model d n_pts regime sigma")
REGIMES = ("benign", "stiff")
MODELS = ("NONE", "OU", "DW", "L63", "L96")
BASE_THETA = {"NONE": [], "OU": [2.0], "DW": [1.0], "L63": [10.0, 28.0, 2.667], "L96": [8.0]}
CENTRE = {"NONE": 1.0, "OU": 0.3, "DW": 1.0, "L63": 1.0, "L96": 8.0}


def _model_of(d):
    return {1: "OU", 2: "NONE", 3: "L63"}.get(d, "L96")


def _n_pts(d):
    return 21 if d <= 17 else 9


# D = 1 .. 4: k_sample_small (D = 2 exists on a "NONE" context alone); 5 .. 64: k_sample_mfma<16 | 32 | 48 | 64>, both sides of every NT
POSTERIOR_WALKS = ([Walk("posterior", _model_of(d), d, _n_pts(d), r, "diag") for d in (1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64) for r in REGIMES] +
                   [Walk("posterior", _model_of(d), d, _n_pts(d), r, "dense") for d in (3, 12, 40) for r in REGIMES])
# the lane kernel (D <= 4) and k_sample_l96 (5 <= D <= 64), the latter also with a dense factor
MODEL_WALKS = ([Walk("model", m, d, 21, "benign", "diag") for m, d in (("OU", 1), ("DW", 1), ("L63", 3), ("L96", 4), ("L96", 5), ("L96", 12), ("L96", 40),
                                                                       ("L96", 64))] + [Walk("model", "L96", 12, 21, "benign", "dense")])
NORMAL_DIMS = (1, 3, 4, 5, 17, 33, 64)      # k_sample_small: 1, 3, 4; k_sample_mfma<16 | 32 | 48 | 64>: 5, 17, 33, 64; an odd D drops half a pair
BIG_NORMALS = Walk("posterior", "L96", 4, 2, "benign", "diag")      # the one large case: 65 536 paths, so that the extremes occur
BIG_PATHS = 65536
START_DIMS = (3, 12)                        # k_pf_start


def walk_id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def walk_inputs(c):
    """the inputs of a walk context (read-only): theta (B, n_theta), sigma (B, D, D), fac = chol_lower(sigma dt) (B, D, D), m0 (D,), s0 (D, D),
    A (B, Np, D, D), b (B, Np, D), x (B, Np D (D + 1)), and one observation (index 1, at the centre, unit noise) for the contexts that want one"""
    d, n = c.d, c.n_pts
    rng = np.random.default_rng([d, n, REGIMES.index(c.regime), int(c.sigma == "dense"), int(c.kind == "model"), MODELS.index(c.model)])
    theta = np.array([[t * (1.0 + 0.05 * k) for t in BASE_THETA[c.model]] for k in range(B)]).reshape(B, -1)
    if c.sigma == "dense":
        sigma = np.stack([spd(rng, d, 4.0) * (1.0 + 0.05 * k) for k in range(B)])
    elif d == 1:
        sigma = np.array([0.8 * (1.0 + 0.1 * k) for k in range(B)]).reshape(B, 1, 1)
    else:
        sigma = np.stack([np.diag(3.0 + rng.random(d)) * (1.0 + 0.1 * k) for k in range(B)])
    if c.model == "NONE":      # (a context without a stochastic model takes no per-problem parameters: its three problems share Sigma)
        sigma = np.stack([sigma[0]] * B)
    m0 = CENTRE[c.model] + 0.5 * rng.standard_normal(d)
    a0 = {"L96": 8.0, "L63": 20.0}.get(c.model, 1.6)
    lin_a, off_b = [], []
    for k in range(B):
        if c.regime == "benign":
            lin_a.append(a0 * np.eye(d) + 0.05 * rng.standard_normal((n, d, d)))
            off_b.append(a0 * m0 + rng.standard_normal((n, d)))
        else:
            a, b = stiff_ab(rng, d, n, "euler")
            lin_a.append(a)
            off_b.append(b)
    lin_a, off_b = np.stack(lin_a), np.stack(off_b)
    out = types.SimpleNamespace(theta=theta, sigma=sigma, fac=np.linalg.cholesky(sigma * DT), m0=m0, s0=0.2 * np.eye(d), A=lin_a, b=off_b,
                                x=np.concatenate((lin_a.reshape(B, -1), off_b.reshape(B, -1)), axis=1),
                                obs_t=np.array([1], dtype=np.int64), obs_y=np.full((1, d), CENTRE[c.model]), obs_noise=np.eye(d))
    for v in vars(out).values():
        v.setflags(write=False)
    return out


def theta_of(c, k):
    th = walk_inputs(c).theta[k]
    return th if th.size > 1 else (float(th[0]) if th.size else 0.0)


def walk_fields(c, k, identity_start=False):
    """problem k of a walk context as the numpy recursions read it"""
    inp = walk_inputs(c)
    return types.SimpleNamespace(model=c.model, dim_d=c.d, n_pts=c.n_pts, dt=DT, theta=theta_of(c, k), sigma=inp.sigma[k],
                                 m0=np.zeros(c.d) if identity_start else inp.m0, s0=np.eye(c.d) if identity_start else inp.s0)


def restated_steps(prev, ks, words, problem, seed, fac, drift, T, drift_scale=None, dt=DT):
    """Every step at once: prev (n, K, D) the states the steps start from, ks (K,) the grid indices they draw at, words (n,) or (n, K) the counter
    words; drift(x, T) -> (f, sum |terms|).  Returns (x (n, K, D), size)."""
    words = np.asarray(words)
    xi, rho = xr.normals(seed, np.asarray(ks)[None, :], words[:, None] if words.ndim == 1 else words, problem, prev.shape[-1], T)
    f, fa = drift(prev, T)
    if drift_scale is not None:
        f = f * T(drift_scale)
    return xr.em_step(prev, f, fa, dt, fac, xi, T, xi_size=XI_SIZE * rho)


def walk_drift(c, k):
    inp = walk_inputs(c)
    if c.kind == "posterior":
        return lambda x, T: xr.posterior_drift(inp.A[k][:-1], inp.b[k][:-1], x, T)
    return lambda x, T: xr.model_drift(c.model, theta_of(c, k), x, T)


def check_steps(worst, label, family, prev, new, ks, words, problem, seed, fac, drift, dt=DT):
    ext, size = restated_steps(prev, ks, words, problem, seed, fac, drift, LD, dt=dt)
    orc, _ = restated_steps(prev, ks, words, problem, seed, fac, drift, F64, dt=dt)
    return record(worst, family, "step", label, new, ext, orc, size)


def check_walk(worst, label, family, c, k, paths):
    """every consecutive pair of problem k's stored stride-1 paths (n, Np, D), drawn with the paths' own indices as counter words"""
    assert paths.shape[1:] == (c.n_pts, c.d) and np.all(np.isfinite(paths)), label
    return check_steps(worst, label, family, paths[:, :-1], paths[:, 1:], np.arange(1, c.n_pts), np.arange(paths.shape[0]), k, SEED,
                       walk_inputs(c).fac[k], walk_drift(c, k))


def check_normals(worst, label, family, got, seed, k, words, problem, d):
    """got (n, D): the device's xi of counter (k, word, problem, .)"""
    ext, rho = xr.normals(seed, k, words, problem, d, LD)
    orc, _ = xr.normals(seed, k, words, problem, d, F64)
    return record(worst, family, "xi", label, got, ext, orc, XI_SIZE * rho)


# ---- B: the forecast from a host-given cloud -----------------------------------------------------------------------------------------------
Forecast = collections.namedtuple("Forecast", "model d n horizon")
FORECAST_INDEX0 = 7
FORECAST_CASES = ([Forecast(m, d, n, h) for m, d in (("OU", 1), ("DW", 1), ("L63", 3), ("L96", 4)) for n in (255, 256, 257) for h in (1, 3)] +
                  [Forecast("L96", d, n, h) for d in (5, 12, 40, 64) for n in (63, 64, 65) for h in (1, 3)])


@functools.lru_cache(maxsize=None)
def forecast_inputs(c):
    """theta (B, n_theta), diagonal sigma (B, D, D), fac, cloud (B, n, D), log_w (B, n) of a forecast case (read-only)"""
    d = c.d
    rng = np.random.default_rng([d, c.n, MODELS.index(c.model), 3])
    theta = np.array([[t * (1.0 + 0.05 * k) for t in BASE_THETA[c.model]] for k in range(B)]).reshape(B, -1)
    sigma = np.stack([np.diag(0.8 + rng.random(d)) * (1.0 + 0.1 * k) for k in range(B)])
    cloud = CENTRE[c.model] + rng.standard_normal((B, c.n, d))
    out = types.SimpleNamespace(theta=theta, sigma=sigma, fac=np.linalg.cholesky(sigma * DT), cloud=cloud, log_w=-7.0 + 3.0 * rng.standard_normal((B, c.n)))
    for v in vars(out).values():
        v.setflags(write=False)
    return out


def forecast_theta(c, k):
    th = forecast_inputs(c).theta[k]
    return th if th.size > 1 else float(th[0])


def check_forecast(worst, label, c, k, members, state_end):
    """members (n, H + 1, D) of the slots 0 .. n - 1 at stride 1 and state_end (n, D) of problem k: the members start at the cloud bit for bit,
    every consecutive pair is one step, and state_end is one step from the members' last point but one"""
    inp = forecast_inputs(c)
    assert np.array_equal(members[:, 0], inp.cloud[k]), label
    assert np.all(np.isfinite(members)) and np.all(np.isfinite(state_end)), label
    drift = lambda x, T: xr.model_drift(c.model, forecast_theta(c, k), x, T)      # noqa: E731
    ks, words = FORECAST_INDEX0 + np.arange(1, c.horizon + 1), np.arange(c.n)
    fails = check_steps(worst, label + " members", "forecast", members[:, :-1], members[:, 1:], ks, words, k, SEED, inp.fac[k], drift)
    return fails + check_steps(worst, label + " state_end", "forecast", members[:, -2:-1], state_end[:, None, :], ks[-1:], words, k, SEED, inp.fac[k], drift)


# ---- C, D: the sums over stored paths ------------------------------------------------------------------------------------------------------------
SEED_W = 77
WEIGHT_SIZES = (17, 65)
STATS_TAGS = ["ou_euler", "dw_euler_p", "l63_euler_p", "l96d4", "l96d5", "l96d12_euler_p", "l96d40_rk4_p"]
# (tag, start, n, ess_fraction) at test_particle_filter_cpu.SEED: the runs of its margin condition in which something is resampled and at
# least two lineages reach stretch 0 (the other fixtures collapse to one survivor: their sums would be trivial)
RESAMPLED_RUNS = [(t, "given", 65, 0.5) for t in ("ou_euler", "dw_euler_p", "l63_euler_p", "l96d4", "l96d17_rk4_p", "quiet_l96d12", "quiet_l96d17",
                                                    "quiet_l96d40")]
# ... and at 300 particles (two 256-slot passes, five workgroups of 64 paths) for the smoothing sums
SMOOTHING_RUNS = RESAMPLED_RUNS + [(t, "given", 300, 0.5) for t in ("ou_euler", "l96d4", "quiet_l96d12", "quiet_l96d40")]


OBS_VARIANTS = [("L63", 3), ("L96", 12)]
SMOOTHING_TAGS = ["l63_euler_p", "l96d5", "l96d12_euler_p", "l96d33", "l96d40_rk4_p", "l96d64"]      # k_sample_small<3>, k_sample_mfma<16 | 16 | 48 | 48 | 64>
SMOOTHING_STRIDES = (1, 4)


@functools.lru_cache(maxsize=None)
def obs_variant(model, d):
    """(problem, x): 41 grid points, observations at the grid indices 0, 1 (adjacent), 20, 21 and Np - 1, a dense R of condition 1e4 and
    H = I + 0.1 noise"""
    import dataclasses
    q, x = make_problem(model, d, 41, method="euler", obs_at=[0, 1, 20, 21, 40])
    if model == "L63":          # (as in test_path_weights.py: keep the Lorenz-63 chain near its data)
        x = np.concatenate((x[:41 * 9], (20.0 * np.asarray(q.m0))[None, :].repeat(41, axis=0).ravel()))
    rng = np.random.default_rng([d, 8])
    return dataclasses.replace(q, obs_noise=xr.spd_with_spectrum(rng, d, 1e4, top=1.0), obs_h=np.eye(d) + 0.1 * rng.standard_normal((d, d))), x


@functools.lru_cache(maxsize=None)
def smoothing_case(tag):
    """(problem, x, given start): test_particle_filter_cpu.case, and "l96d33" built the way its "l96d5" is"""
    if tag == "l96d33":
        q, x = make_problem("L96", 33, 41, method="euler")
        return q, x, np.reshape(np.asarray(q.m0, dtype=float), 33) + 0.1
    return case(tag)


def check_smoothing(worst, label, family, log_w, table, paths, stride, mean, second, lineage_ess):
    """The sums of the replay from the lineages (n, Np, D) of particle_paths(slots=arange(n), stride=1), the final log-weights and the slot table
    (M + 1, n): mean (n_keep, D) = sum_m W_m paths[m][k], second (n_keep, D) or (n_keep, D, D) = sum_m W_m x^2 or x x^T,
    lineage_ess[j] = 1 / sum_a (W^j_a)^2 with W^j_a = sum_{m: s_j[m] = a} W_m, its size (1 + max |lw - max lw|) times the value"""
    kept = np.asarray(paths)[:, ::stride]
    fails = check_weighted_sum(worst, label, family, "sum W x", log_w, kept, mean)
    if np.ndim(second) == 3:      # (the products x x^T a few kept indices at a time: 257 lineages at D = 64 would not fit at once)
        step = max(1, 2 ** 22 // (kept.shape[0] * kept.shape[2] ** 2))
        parts = []
        for k0 in range(0, kept.shape[1], step):
            blk = kept[:, k0:k0 + step].astype(LD)
            sq = np.einsum("nka,nkb->nkab", blk, blk)
            parts.append(xr.weighted_sum(log_w, sq, LD) + (xr.weighted_sum(log_w, sq, F64)[0],))
        ext, size, orc = (np.concatenate(v) for v in zip(*parts))
        fails += record(worst, family, "sum W x x^T", label, second, ext, orc, size)
    else:
        fails += check_weighted_sum(worst, label, family, "sum W x^2", log_w, kept.astype(LD) ** 2, second)
    out = {}
    for T in (LD, F64):
        out[T] = 1 / xr._sum(xr.stretch_weights(log_w, table, T) ** 2, -1)
    spread = 1 + np.max(np.abs(np.asarray(log_w, dtype=LD) - np.max(log_w))) + 2 * xr.levels(np.size(log_w))      # (+ the two sums' additions, as in weighted_sum)
    return fails + record(worst, family, "lineage_ess", label, lineage_ess, out[LD], out[F64], spread * out[LD])


# backward simulation: runs of RESAMPLED_RUNS, and the tight clouds of test_particle_backward_cpu, where the drawn slot is not the ancestor
BACKWARD_RUNS = RESAMPLED_RUNS[:4] + [("quiet_l96d12", "given", 65, 0.5), ("tight12", "drawn", 65, 1.0), ("tight40", "drawn", 65, 1.0)]


def backward_case(tag):
    """(problem, x, given start or None)"""
    if tag.startswith("tight"):
        from test_particle_backward_cpu import tight_case
        return tight_case(int(tag[5:])) + (None,)
    return case(tag)


def backward_prev(paths, table, obs_t, ancestors, clouds):
    """(n, Np - 1, D): the state every step of a backward-simulation walk starts from -- the stored point, but behind a completed observation j
    the particle the walk's next slot was copied from, clouds[j][ancestors[j][table[j + 1]]], out of the filter's history"""
    prev = np.array(paths[:, :-1])
    for j, t in enumerate(np.asarray(obs_t, dtype=np.int64).ravel()):
        if t < paths.shape[1] - 1:
            prev[:, t] = np.asarray(clouds)[j][np.asarray(ancestors)[j][np.asarray(table)[j + 1]]]
    return prev


def check_backward(worst, label, family, q, x, paths, table, ancestors, clouds, seed):
    """every step of the backward-simulation trajectories (n, Np, D) of one problem"""
    d, n_pts = int(q.dim_d), int(q.n_pts)
    lin_a, off_b = _split(q, x)
    drift = lambda v, T: xr.posterior_drift(lin_a.reshape(-1, d, d)[:-1], off_b.reshape(-1, d)[:-1], v, T)      # noqa: E731
    fac = np.linalg.cholesky(_sigma_diag(q) * float(q.dt))
    prev = backward_prev(paths, table, q.obs_t, ancestors, clouds)
    return check_steps(worst, label, family, prev, paths[:, 1:], np.arange(1, n_pts), lineage_words(q.obs_t, table, n_pts), 0, seed, fac, drift,
                       dt=float(q.dt))


def _theta(q):
    th = np.asarray(q.theta, dtype=float)
    return th if th.ndim else float(th)


def check_weights(worst, label, family, q, x, paths, path_got, obs_got):
    """the two sums of the stored stride-1 paths (n, Np, D) of problem q; obs_got None: the path term alone"""
    lin_a, off_b = _split(q, x)
    sd = _sigma_diag(q).diagonal()
    args = (q.model, _theta(q), sd, float(q.dt), lin_a.reshape(q.n_pts, q.dim_d, q.dim_d), off_b.reshape(q.n_pts, q.dim_d), paths)
    ext, scale, rec = xr.path_term(*args, T=LD)
    orc, _, _ = xr.path_term(*args, T=F64)
    fails = record(worst, family, "path term", label, path_got, ext, orc, scale + rec)
    if obs_got is not None:
        oargs = (q.obs_t, q.obs_y, q.obs_noise, getattr(q, "obs_h", None), paths)
        ext, size = xr.obs_term(*oargs, T=LD)
        orc, _ = xr.obs_term(*oargs, T=F64)
        fails += record(worst, family, "obs term", label, obs_got, ext, orc, size)
    return fails


def check_log_weights(worst, label, q, x, paths, log_w):
    """particle_filter(ess_fraction=0) from a given start: log_w = -c + path + obs of the stored paths, the size the sum of the two terms' sizes"""
    lin_a, off_b = _split(q, x)
    args = (q.model, _theta(q), _sigma_diag(q).diagonal(), float(q.dt), lin_a.reshape(q.n_pts, q.dim_d, q.dim_d), off_b.reshape(q.n_pts, q.dim_d), paths)
    oargs = (q.obs_t, q.obs_y, q.obs_noise, getattr(q, "obs_h", None), paths)
    out = {}
    for T in (LD, F64):
        pt, scale, rec = xr.path_term(*args, T=T)
        ot, size = xr.obs_term(*oargs, T=T)
        out[T] = (pt + ot, scale + rec + size)
    return record(worst, "filter", "log_w", label, log_w, out[LD][0], out[F64][0], out[LD][1])


def check_rows(worst, label, family, q, paths, rows):
    """the rows (n, 3, D) of path statistics against the restatement on the stored paths or lineages (n, Np, D)"""
    args = (q.model, _theta(q), float(q.dt), paths)
    ext, size = xr.statistics_rows(*args, T=LD)
    orc, _ = xr.statistics_rows(*args, T=F64)
    fails = []
    for s, name in enumerate(("Q", "G", "H")):
        if name == "H" and q.dim_d >= 5:      # the constant dt (Np - 1), written and not summed
            exact = np.all(np.asarray(rows)[:, 2] == float(q.dt) * float(q.n_pts - 1))
            print(f"{label} [{family}] H: the constant dt (Np - 1), equal: {bool(exact)}")
            fails += [] if exact else [(label, family, "H", 0.0, np.inf)]
        else:
            fails += record(worst, family, name, label, np.asarray(rows)[:, s], ext[:, s], orc[:, s], size[:, s])
    return fails


def check_weighted_sum(worst, label, family, quantity, log_w, values, got):
    ext, size = xr.weighted_sum(log_w, values, LD)
    orc, _ = xr.weighted_sum(log_w, values, F64)
    return record(worst, family, quantity, label, got, ext, orc, size)


# ---- E: the forecast's moments at horizon 0 ------------------------------------------------------------------------------------------------
MOMENT_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
MOMENT_WEIGHTS = ("spread0", "spread5", "spread40", "spread700", "dominant", "offset", "small_mean")
MOMENT_SHAPES = [("OU", 1), ("L63", 3), ("L96", 4), ("L96", 5), ("L96", 40)]      # k_sample_small<1 | 3 | 4, Forecast>, k_forecast_l96


@functools.lru_cache(maxsize=None)
def moment_case(model, d, n, weights):
    """(cloud (n, D), log_w (n,)): log-weights spread over 0, 5, 40 or 700, one dominant weight (the others 40 below), all equal at -1e4, or a
    cloud whose mean is 1e-3 of its spread"""
    rng = np.random.default_rng([d, n, MOMENT_WEIGHTS.index(weights), 4])
    cloud = CENTRE[model] + rng.standard_normal((n, d))
    lw = -7.0 + rng.standard_normal(n)
    if weights.startswith("spread"):
        lw = -3.0 - float(weights[6:]) * rng.permutation(n) / max(n - 1, 1)
    elif weights == "dominant":
        lw[n // 2] += 40.0
    elif weights == "offset":
        lw = np.full(n, -1e4)
    else:
        cloud = 1e-3 + rng.standard_normal((n, d))
    cloud.setflags(write=False)
    lw.setflags(write=False)
    return cloud, lw


def check_moments(worst, label, cloud, log_w, moments):
    """moments (2, D) of a cloud (n, D): sum W x and sum W x^2"""
    fails = check_weighted_sum(worst, label, "forecast moments", "sum W x", log_w, cloud, moments[0])
    return fails + check_weighted_sum(worst, label, "forecast moments", "sum W x^2", log_w, np.asarray(cloud, dtype=LD) ** 2, moments[1])


def lineage_words(obs_t, table, n_pts):
    """(n, Np - 1): the counter word of every lineage at the steps k = 1 .. Np - 1 from the slot table (M + 1, n): step k draws with the slot of
    stretch #{j: t_j < k}"""
    stretch = np.searchsorted(np.sort(np.asarray(obs_t, dtype=np.int64)), np.arange(1, n_pts), side="left")
    return np.asarray(table)[stretch].T


# ================================================================================================================================== tests
def test_tables_cover_what_they_name():
    assert {c.d for c in POSTERIOR_WALKS if c.sigma == "diag"} == {1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64}
    assert {c.d for c in POSTERIOR_WALKS if c.sigma == "dense"} == {3, 12, 40}
    assert all({c.regime for c in POSTERIOR_WALKS if c.d == d} == set(REGIMES) for d in {c.d for c in POSTERIOR_WALKS})
    assert {(c.model, c.d) for c in MODEL_WALKS} == {("OU", 1), ("DW", 1), ("L63", 3), ("L96", 4), ("L96", 5), ("L96", 12), ("L96", 40), ("L96", 64)}
    assert all(c.n_pts <= 21 for c in POSTERIOR_WALKS + MODEL_WALKS) and N_PATHS <= 65 and B == 3
    assert {(c.d, c.n) for c in FORECAST_CASES} == {(d, n) for d in (1, 3, 4) for n in (255, 256, 257)} | {(d, n) for d in (5, 12, 40, 64) for n in (63, 64, 65)}
    assert {c.horizon for c in FORECAST_CASES} == {1, 3} and {c.model for c in FORECAST_CASES if c.d == 1} == {"OU", "DW"}
    assert max(MOMENT_SIZES) <= 513


@pytest.mark.parametrize("c", [c for c in POSTERIOR_WALKS if c.regime == "stiff"], ids=walk_id)
def test_stiff_regime(c):
    """dt rho(A_t) = 0.45 at every grid point of every problem: the drift is a large share of s_i"""
    inp = walk_inputs(c)
    rho = DT * np.max(np.abs(np.linalg.eigvals(inp.A)), axis=-1)
    assert np.all(rho >= 0.4) and np.all(rho <= 1.0), (rho.min(), rho.max())
    assert np.allclose(rho, 0.45, rtol=1e-10)


def test_the_large_normals_case_contains_the_extremes():
    """from the host's Philox alone: among the compared uniforms are u1 < 1e-4, 1 - u1 < 1e-4 and u2 within 1e-4 of 0, 1/4, 1/2, 3/4"""
    u1, u2 = xr.uniforms(SEED, 0, np.arange(BIG_PATHS), 0, BIG_NORMALS.d)
    assert u1.shape == (BIG_PATHS, 2)
    assert u1.min() < 1e-4 and 1.0 - u1.max() < 1e-4
    assert min(u2.min(), 1.0 - u2.max()) < 1e-4
    for c in (0.25, 0.5, 0.75):
        assert np.min(np.abs(u2 - c)) < 1e-4, c
    print("u1 in [", u1.min(), ",", u1.max(), "]; largest rho", float(np.sqrt(-2.0 * np.log(u1.min()))))


def test_normals_floor_covers_the_oracle():
    """numpy's Box-Muller in the device's place, the large case included"""
    from test_sample_paths_cpu import normals as normals_numpy
    fails = []
    with floor_covers_the_oracle():
        for d in NORMAL_DIMS:
            for p in range(B):
                got = normals_numpy(SEED, 0, np.arange(N_PATHS), p, d)
                fails += check_normals(WORST, f"D={d} p={p}", "cpu normals", got, SEED, 0, np.arange(N_PATHS), p, d)
        got = normals_numpy(SEED, 0, np.arange(BIG_PATHS), 0, BIG_NORMALS.d)
        fails += check_normals(WORST, "65536 paths", "cpu normals", got, SEED, 0, np.arange(BIG_PATHS), 0, BIG_NORMALS.d)
    assert not fails, fails


@pytest.mark.parametrize("c", POSTERIOR_WALKS + MODEL_WALKS, ids=walk_id)
def test_step_floor_covers_the_oracle(c):
    """sample_paths_numpy in the device's place: every step of every path of the three problems within the floor; no overflow"""
    for k in range(B):
        q = walk_fields(c, k)
        paths = sample_paths_numpy(q, c.kind, walk_inputs(c).x[k] if c.kind == "posterior" else None, None, N_PATHS, 1, SEED, index=k)
        with floor_covers_the_oracle():
            assert not check_walk(WORST, f"{walk_id(c)} p={k}", "cpu " + c.kind, c, k, paths)
        assert np.max(np.abs(paths)) < 1e6


@pytest.mark.parametrize("c", FORECAST_CASES, ids=walk_id)
def test_forecast_floor_covers_the_oracle(c):
    inp = forecast_inputs(c)
    for k in range(B):
        q = types.SimpleNamespace(model=c.model, dim_d=c.d, dt=DT, theta=forecast_theta(c, k), sigma=inp.sigma[k])
        ref = forecast_numpy(q, inp.cloud[k], inp.log_w[k], FORECAST_INDEX0, c.horizon, 1, SEED, np.arange(c.n), index=k)
        assert np.array_equal(ref["members"][:, -1], ref["state_end"])
        with floor_covers_the_oracle():
            assert not check_forecast(WORST, f"{walk_id(c)} p={k}", c, k, ref["members"], ref["state_end"])


@pytest.mark.parametrize("tag", TAGS)
def test_weight_floors_cover_the_oracle(tag):
    """path_weights_numpy's two sums against the restatement on sample_paths_numpy's stored paths: given and drawn start"""
    q, x, x0 = case(tag)
    for start in (x0, None):
        stored = sample_paths_numpy(q, "posterior", x, start, 17, 1, SEED_W)
        _, path, obs, _ = path_weights_numpy(q, x, start, 17, SEED_W)
        with floor_covers_the_oracle():
            assert not check_weights(WORST, f"{tag} {'given' if start is not None else 'drawn'}", "cpu weights", q, x, stored, path, obs)


@pytest.mark.parametrize("model,d", OBS_VARIANTS)
def test_obs_variant_floors_cover_the_oracle(model, d):
    q, x = obs_variant(model, d)
    assert np.linalg.cond(q.obs_noise) == pytest.approx(1e4, rel=1e-6) and list(q.obs_t) == [0, 1, 20, 21, 40] and q.n_pts == 41
    stored = sample_paths_numpy(q, "posterior", x, None, 17, 1, SEED_W)
    _, path, obs, _ = path_weights_numpy(q, x, None, 17, SEED_W)
    with floor_covers_the_oracle():
        assert not check_weights(WORST, f"{model}{d} dense R, H", "cpu weights dense R", q, x, stored, path, obs)


@pytest.mark.parametrize("run", SMOOTHING_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_smoothing_floors_cover_the_oracle(run):
    """the restated lineages, reweighted with numpy, in the device's place"""
    tag, start, n, frac = run
    ref = paths_reference(tag, start, n, frac)
    w = np.exp(ref["lw"] - ref["lw"].max())
    w /= w.sum()
    paths = ref["paths"]
    wj = np.stack([np.bincount(row, weights=w, minlength=n) for row in ref["table"]])
    with floor_covers_the_oracle():
        for stride in SMOOTHING_STRIDES:
            kept = paths[:, ::stride]
            assert not check_smoothing(WORST, f"{tag} stride {stride}", "cpu smoothing", ref["lw"], ref["table"], paths, stride,
                                       np.einsum("n,nka->ka", w, kept), np.einsum("n,nka,nkb->kab", w, kept, kept), 1.0 / np.sum(wj * wj, axis=1))


@pytest.mark.parametrize("tag", STATS_TAGS)
def test_row_floors_cover_the_oracle(tag):
    """particle_statistics_numpy(ess_fraction=0)'s rows against the restatement on the stored paths; the mean of the rows as one reduction"""
    q, x, x0 = case(tag)
    stored = sample_paths_numpy(q, "posterior", x, x0, 17, 1, PF_SEED)
    ref = particle_statistics_numpy(q, x, x0, 17, PF_SEED, 0.0)
    assert np.array_equal(ref["state"], stored[:, -1])
    rows = ref["rows"].copy()
    if q.dim_d >= 5:
        rows[:, 2] = float(q.dt) * float(q.n_pts - 1)      # (the device writes the constant; numpy sums dt forty times)
    with floor_covers_the_oracle():
        assert not check_rows(WORST, tag, "cpu rows", q, stored, rows)
        w = np.exp(ref["lw"] - ref["lw"].max())
        mean = np.tensordot(w, rows, axes=(0, 0)) / w.sum()
        assert not check_weighted_sum(WORST, tag, "cpu rows", "mean of rows", ref["lw"], rows, mean)


@pytest.mark.parametrize("run", SMOOTHING_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_resampled_runs_are_not_trivial(run):
    """something is resampled, at least two distinct lineages reach stretch 0, and every step of the restated lineages is one step of the
    recursion drawn with the word of lineage_words (the numpy re-walk in the device's place)"""
    tag, start, n, frac = run
    q, x, x0 = case(tag)
    ref = paths_reference(tag, start, n, frac)
    assert ref["resampled"].any() and len(set(ref["table"][0].tolist())) >= 2
    assert min(ref["margins"]) >= 1e-7
    lin_a, off_b = _split(q, x)
    d = int(q.dim_d)
    paths = ref["paths"]
    words = lineage_words(ref["obs_t"], ref["table"], int(q.n_pts))
    drift = lambda v, T: xr.posterior_drift(lin_a.reshape(-1, d, d)[:-1], off_b.reshape(-1, d)[:-1], v, T)      # noqa: E731
    fac = np.linalg.cholesky(_sigma_diag(q) * float(q.dt))
    with floor_covers_the_oracle():
        assert not check_steps(WORST, tag, "cpu lineage", paths[:, :-1], paths[:, 1:], np.arange(1, int(q.n_pts)), words, 0, PF_SEED, fac, drift)


@pytest.mark.parametrize("run", BACKWARD_RUNS, ids=lambda r: f"{r[0]}-{r[2]}-{r[3]}")
def test_backward_step_floor_covers_the_oracle(run):
    """the numpy backward simulation and its re-walk in the device's place; in the tight cases a reload replaces the state by another particle"""
    from test_particle_backward_cpu import backward_slots_numpy, history_numpy, rewalk_backward_numpy
    tag, start, n, frac = run
    q, x, x0 = backward_case(tag)
    hist = history_numpy(q, x, x0, n, PF_SEED, frac)
    assert hist["resampled"].any()
    table, _ = backward_slots_numpy(q, x, PF_SEED, hist, np.arange(n))
    paths = rewalk_backward_numpy(q, x, x0, PF_SEED, table, hist)
    prev = backward_prev(paths, table, q.obs_t, hist["ancestors"], hist["clouds"])
    if tag.startswith("tight"):
        assert not np.array_equal(prev, paths[:, :-1])
    with floor_covers_the_oracle():
        assert not check_backward(WORST, tag, "cpu backward", q, x, paths, table, hist["ancestors"], hist["clouds"], PF_SEED)


@pytest.mark.parametrize("model,d", MOMENT_SHAPES)
def test_moment_floors_cover_the_oracle(model, d):
    for n in MOMENT_SIZES:
        for weights in MOMENT_WEIGHTS:
            cloud, lw = moment_case(model, d, n, weights)
            w = np.exp(lw - lw.max())
            assert np.all(np.isfinite(w)) and w.sum() >= 1.0
            if weights == "spread700" and n > 1:
                assert np.count_nonzero(w) >= 2 and (lw.max() - lw.min()) == pytest.approx(700.0)
            if weights == "small_mean" and n >= 63:
                assert abs(cloud.mean()) <= 0.5 * cloud.std()
            w = w / w.sum()
            with floor_covers_the_oracle():
                assert not check_moments(WORST, f"{model}{d} n={n} {weights}", cloud, lw, np.stack((w @ cloud, w @ (cloud * cloud))))


# ---- the mutants: each passes the older check's measure and misses the new bound -----------------------------------------------------------------
MUT = 1.0 + 2.0 ** -30


def _missed(e_k, e_o):
    return e_k / (FACTOR * max(e_o, 1.0))


def test_mutants():
    """factor: e_k over the right-hand side of the bound (> 1: the bound is missed).  old: the mutant on the measure of the older check."""
    report = {}
    # 1. dt (1 + 2^-30) in the quadratic term of the path increment -- older measure |got - want| / (1 + scale) <= 1e-9 (test_path_weights.py)
    for tag in ("l63_euler_p", "l96d12_euler_p", "l96d40_rk4_p"):
        q, x, x0 = case(tag)
        stored = sample_paths_numpy(q, "posterior", x, None, 17, 1, SEED_W)
        _, path, _, scale = path_weights_numpy(q, x, None, 17, SEED_W)
        lin_a, off_b = _split(q, x)
        d, n = int(q.dim_d), int(q.n_pts)
        args = (q.model, _theta(q), _sigma_diag(q).diagonal(), float(q.dt), lin_a.reshape(n, d, d), off_b.reshape(n, d), stored)
        ext, sc, rec = xr.path_term(*args, T=LD)
        orc, _, _ = xr.path_term(*args, T=F64)
        prev = stored[:, :-1]
        g = off_b.reshape(n, d)[:-1] - np.einsum("kij,nkj->nki", lin_a.reshape(n, d, d)[:-1], prev)
        f, _ = xr.model_drift(q.model, _theta(q), prev, F64)
        dd = g - f
        quad = 0.5 * float(q.dt) * np.sum(dd * dd / _sigma_diag(q).diagonal(), axis=(-1, -2))
        mutant = path - (MUT - 1.0) * quad
        e_k, e_o = errors(mutant, ext, orc, sc + rec)
        old = float(np.max(np.abs(mutant - path) / (1.0 + scale)))
        report["quadratic dt, " + tag] = (old, _missed(e_k, e_o))
        # the older check passes it on Lorenz-63 (9.6e-10) and stands at its tolerance on the two Lorenz-96 fixtures (1.01e-9, 1.03e-9: it
        # rejects them by a margin that is noise to it) -- the first is asserted, the others are reported
        assert (old <= 1e-9 if tag == "l63_euler_p" else 1e-9 < old <= 1.1e-9) and not within(e_k, e_o)
    # 2. the drift of one step times 1 + 2^-30 -- older measure conftest.rel_err <= 1e-9 (test_sample_paths.py)
    for c in (Walk("posterior", "L96", 12, 21, "benign", "diag"), Walk("posterior", "L96", 40, 9, "stiff", "dense"), Walk("model", "L96", 12, 21, "benign", "diag")):
        q = walk_fields(c, 1)
        paths = sample_paths_numpy(q, c.kind, walk_inputs(c).x[1] if c.kind == "posterior" else None, None, N_PATHS, 1, SEED, index=1)
        args = (paths[:, :-1], np.arange(1, c.n_pts), np.arange(N_PATHS), 1, SEED, walk_inputs(c).fac[1], walk_drift(c, 1))
        ext, size = restated_steps(*args, LD)
        orc, _ = restated_steps(*args, F64)
        mutant, _ = restated_steps(*args, F64, drift_scale=MUT)
        e_k, e_o = errors(mutant, ext, orc, size)
        old = rel_err(mutant, paths[:, 1:])
        report["drift, " + walk_id(c)] = (old, _missed(e_k, e_o))
        assert old <= 1e-9 and not within(e_k, e_o)
    # 3. r^2 (1 / dt) with 1 / dt off by 2^-30 in Q -- older measure |got - want| <= 1e-9 scale, scale = sum |summand| (test_particle_statistics.py)
    for tag in ("l63_euler_p", "l96d12_euler_p"):
        q, x, x0 = case(tag)
        stored = sample_paths_numpy(q, "posterior", x, x0, 17, 1, PF_SEED)
        ref = particle_statistics_numpy(q, x, x0, 17, PF_SEED, 0.0)
        ext, size = xr.statistics_rows(q.model, _theta(q), float(q.dt), stored, T=LD)
        orc, _ = xr.statistics_rows(q.model, _theta(q), float(q.dt), stored, T=F64)
        mutant = ref["rows"][:, 0] * MUT
        e_k, e_o = errors(mutant, ext[:, 0], orc[:, 0], size[:, 0])
        old = float(np.max(np.abs(mutant - ref["rows"][:, 0]) / ref["scale"][:, 0]))
        report["1 / dt in Q, " + tag] = (old, _missed(e_k, e_o))
        assert old <= 1e-9 and not within(e_k, e_o)
    # 4. weights normalised by S (1 + 2^-30) -- older measure 1e-9 sum W |x| (test_particle_forecast.py)
    for model, d, n, weights in (("L96", 5, 257, "spread5"), ("L96", 40, 513, "dominant"), ("L63", 3, 65, "spread40")):
        cloud, lw = moment_case(model, d, n, weights)
        ext, size = xr.weighted_sum(lw, cloud, LD)
        orc, _ = xr.weighted_sum(lw, cloud, F64)
        mutant, _ = xr.weighted_sum(lw, cloud, F64, total_scale=MUT)
        e_k, e_o = errors(mutant, ext, orc, size)
        w = np.exp(lw - lw.max())
        old = float(np.max(np.abs(mutant - orc) / ((w / w.sum()) @ np.abs(cloud))))
        report[f"weight sum, {model}{d} n={n} {weights}"] = (old, _missed(e_k, e_o))
        assert old <= 1e-9 and not within(e_k, e_o)
    # 5. xi with the fp32 value of 2 pi: the angle is off by up to 1.7e-7, which the generator check of test_sample_paths.py (1e-12 absolute)
    #    sees, and so does the paths' measure (8.2e-9 against rel_err <= 1e-9): the one mutant of the five that the older checks reject too --
    #    asserted as such; it is kept because the new bound misses it by the widest margin of all, not because it was hidden
    c = Walk("posterior", "L96", 12, 21, "benign", "diag")
    ext, rho = xr.normals(SEED, 0, np.arange(N_PATHS), 0, c.d, LD)
    orc, _ = xr.normals(SEED, 0, np.arange(N_PATHS), 0, c.d, F64)
    mutant, _ = xr.normals(SEED, 0, np.arange(N_PATHS), 0, c.d, F64, angle=float(np.float32(2.0 * np.pi)))
    e_k, e_o = errors(mutant, ext, orc, XI_SIZE * rho)
    fac = walk_inputs(c).fac[0]
    old = float(np.max(np.abs((mutant - orc) @ fac.T)) / np.max(np.abs(walk_inputs(c).m0)))
    report["fp32 2 pi"] = (old, _missed(e_k, e_o))
    assert old > 1e-9 and not within(e_k, e_o)
    # 6. dt (1 + 2^-30) inside the implied increment eta* = (ref_k - ref_{k-1}) - dt g of the conditional filter's pinned slot -- older measure
    #    |got - want| <= 1e-9 max |log_w| (test_particle_gibbs.py); the new bound is test_particle_ancestor.py's on log_w[:, 0]
    from test_particle_ancestor_cpu import WEIGHT_SEED, pinned_weight, weight_case, weight_references
    from test_particle_gibbs_cpu import conditional_filter_numpy
    #    On the drawn references, and on the smooth one of the double well, the older check passes it by a factor 10 .. 100; on the smooth
    #    references of the n-D models (eta* some 5 R per step) it stands at 2 .. 4 of its tolerance: asserted as such, as mutant 5 is
    for model, d, kind in (("DW", 1, "smooth"), ("L63", 3, "drawn"), ("L96", 12, "drawn"), ("L96", 40, "drawn"), ("L96", 40, "smooth")):
        probs, xs = weight_case(model, d)
        q, x, ref = probs[1], xs[1], weight_references(model, d, "drawn", kind)[1]
        honest = conditional_filter_numpy(q, x, None, ref, 65, WEIGHT_SEED, 0.0, index=1)["lw"]
        mutant = conditional_filter_numpy(q, x, None, ref, 65, WEIGHT_SEED, 0.0, index=1, eta_dt=float(q.dt) * MUT)["lw"]
        assert np.array_equal(mutant[1:], honest[1:])
        ext, size = pinned_weight(q, x, "drawn", ref, LD)
        orc, _ = pinned_weight(q, x, "drawn", ref, F64)
        e_k, e_o = errors(mutant[0], ext, orc, size)
        old = float(np.max(np.abs(mutant - honest)) / np.max(np.abs(honest)))
        report[f"dt inside eta*, {model}{d} {kind}"] = (old, _missed(e_k, e_o))
        assert (1e-9 < old <= 5e-9 if (d, kind) == (40, "smooth") else old <= 1e-9) and not within(e_k, e_o)
    for name, (old, factor) in report.items():
        print(f"mutant {name}: older measure {old:.2e}, over the new bound by {factor:.3g}x")
        assert factor > 1.0


def test_print_worst():
    """(last: the worst ratio per family and quantity of this run, numpy in the device's place)"""
    for (family, quantity), r in sorted(WORST.items()):
        print(f"WORST {family} / {quantity}: {r:.3f}")
