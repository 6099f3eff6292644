"""
The particle filter's walk in numpy: the ONLY place its arithmetic is spelled.  Every restatement in tests/test_particle_*_cpu.py (the
references of the GPU tests beside them) consumes it and keeps, in its own file, what it carries along the lineages.

The walk is the recursion of test_path_weights_cpu.path_weights_numpy (the same normals, model drift, observation model and initial term)
with n particles per problem.  It takes the observation terms into the log-weights lw where they occur, and behind every observation forms
    w_i = exp(lw_i - max lw),  cum = cumsum(w) in slot order,  S = cum[n - 1],  ESS = S^2 / sum w_i^2
and resamples iff ESS < ess_fraction n and k < Np - 1:
    U = unit_open(r0, r1) of Philox counter (k, 0, problem, 0xffffffff),  u_i = (U + i) / n S,  anc_i = min(#{m: cum_m <= u_i}, n - 1),
    x_i <- x_{anc_i},  lw_i <- max lw + log S - log n.
(S is taken as the last prefix sum, which is sum_i w_i in slot order, so that every threshold lies below cum[n - 1] as it does in exact
arithmetic.)  For each resampling it also records the margin min_{i,m} |u_i - cum_m| / S: device and host weights agree to about 1e-13, so
above a margin of 1e-7 the device's ancestors must be identical to the restatement's -- the condition
test_particle_filter_cpu.test_margin_condition asserts for every (case, n, seed) the GPU tests use.

FilterWalk is an iterator of events over the grid; between two events the consumer reads the walk's attributes and updates what it carries:
    ("start", 0)    state (n, D) and init (n,) are set; nothing is observed yet
    ("step", k)     the step to grid index k is taken: prev (the state before it), dd = g - f at prev, eta = R xi_k, inc (the path term's
                    increment, already in lw), state (after it)
    ("cut", j)      observation j (at grid index obs_t[j]) is in lw; ess[j], clouds[j] and ancestors[j] (the identity) are recorded; the
                    resampling decision is not yet made
    ("gather", j)   the cloud was resampled: anc (n,); state and lw are already the gathered / reset ones, ancestors[j] = anc
A "cut" follows the "start" or "step" of its grid index, a "gather" its "cut".  What is carried through a resampling is gathered as
carried[anc] at "gather".  The consumer leaves the walk's attributes as they are; d, n_pts, dt and obs_t of the problem are among them, and
record() returns the finished walk's dict with what the consumer adds.

The pieces of the observation step (weight_sums, systematic_ancestors, reset_weights) are functions of their own:
test_particle_gibbs_cpu.conditional_filter_numpy composes them with its pinned slot and its own draws.  visited_states is the unweighted
replay of a finished walk through its stored ancestors.
"""
import numpy as np

from test_path_weights_cpu import _sigma_diag, _split, observation_term, obs_model, path_increment, start_term
from test_sample_paths_cpu import em_noise, em_step, model_drift, philox4x32_10, start_cloud, unit_open


def weight_sums(lw):
    """(top, w, cum, S, ESS) of the log-weights behind an observation"""
    top = lw.max()
    w = np.exp(lw - top)
    cum = np.cumsum(w)
    total = cum[-1]
    return top, w, cum, total, total * total / np.sum(w * w)


def systematic_ancestors(cum, total, seed, k, index):
    """(anc (n,), margin): the systematic resampling at grid index k from the prefix sums"""
    n = cum.size
    rr = philox4x32_10((k, 0, index, 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = (float(unit_open(rr[0], rr[1])) + np.arange(n)) / n * total
    pos = np.searchsorted(cum, u, side="right")
    near = np.minimum(np.abs(u - cum[np.minimum(pos, n - 1)]), np.where(pos > 0, np.abs(u - cum[np.maximum(pos - 1, 0)]), np.inf))
    return np.minimum(pos, n - 1), float(near.min() / total)


def reset_weights(top, total, n):
    """(n,): the common log-weight behind a resampling"""
    return np.full(n, top + np.log(total) - np.log(n))


class FilterWalk:
    """One problem's filter with counter word `index` (the module's docstring)."""

    def __init__(self, problem, x, x0, n, seed, ess_fraction, index=0):
        self.problem, self.x, self.x0, self.n, self.seed, self.ess_fraction, self.index = problem, x, x0, n, seed, ess_fraction, index
        self.d, self.n_pts, self.dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
        self.obs_t, self.obs_y, self.q, self.const = obs_model(problem)
        m = self.obs_t.size
        self.ess, self.resampled, self.margins = np.zeros(m), np.zeros(m, dtype=np.int64), []
        self.ancestors, self.clouds = np.full((m, n), -1, dtype=np.int64), np.full((m, n, self.d), np.nan)

    def __iter__(self):
        problem, seed, index, dt = self.problem, self.seed, self.index, self.dt
        sigma = _sigma_diag(problem)
        isg, fac = 1.0 / sigma.diagonal(), np.linalg.cholesky(sigma * dt)
        lin_a, off_b = _split(problem, self.x)
        theta = np.asarray(problem.theta, dtype=float)
        at = {int(t): j for j, t in enumerate(self.obs_t)}
        slots = np.arange(self.n)
        self.state = start_cloud(problem, self.x0, seed, slots, index)
        self.init = start_term(problem, self.state, self.x0)
        self.lw = self.init - self.const
        yield "start", 0
        for k in range(self.n_pts):
            if k > 0:
                self.prev = self.state
                g = -(self.prev @ lin_a[k - 1].T) + off_b[k - 1]
                self.dd = g - model_drift(problem.model, theta, self.prev)
                self.eta = em_noise(seed, k, slots, index, fac)
                self.inc = path_increment(self.dd, self.eta, isg, dt)
                self.lw = self.lw + self.inc
                self.state = em_step(self.prev, dt, g, self.eta)
                yield "step", k
            if k not in at:
                continue
            j = at[k]
            self.lw = self.lw + observation_term(self.obs_y[j], self.state, self.q)
            top, _, cum, total, ess = weight_sums(self.lw)
            self.ess[j], self.clouds[j], self.ancestors[j] = ess, self.state, slots
            yield "cut", j
            if ess < self.ess_fraction * self.n and k < self.n_pts - 1:
                self.anc, margin = systematic_ancestors(cum, total, seed, k, index)
                self.margins.append(margin)
                self.resampled[j], self.ancestors[j] = 1, self.anc
                self.state, self.lw = self.state[self.anc], reset_weights(top, total, self.n)
                yield "gather", j

    def record(self, **more):
        """the finished walk as the dict every restatement returns: lw (n,), state (n, D), ess (M,), resampled (M,) int, ancestors (M, n)
        (the identity where the cloud was carried on), clouds (M, n, D), margins (one per resampling), obs_t (M,), and what the consumer adds"""
        return dict(lw=self.lw, state=self.state, ess=self.ess, resampled=self.resampled, ancestors=self.ancestors, clouds=self.clouds,
                    margins=self.margins, obs_t=np.asarray(self.obs_t, dtype=np.int64), **more)


def visited_states(problem, x, x0, seed, n, gathers, index=0):
    """(visited (Np, n, D), the final state (n, D)): the state of slot i as the walk arrives at k, before a resampling decision at k -- the
    filter's steps without its weights, gathered through gathers[k] (n,) at the grid indices k it names"""
    n_pts, dt = int(problem.n_pts), float(problem.dt)
    fac = np.linalg.cholesky(_sigma_diag(problem) * dt)
    lin_a, off_b = _split(problem, x)
    slots = np.arange(n)
    state = start_cloud(problem, x0, seed, slots, index)
    visited = np.empty((n_pts, n, int(problem.dim_d)))
    for k in range(n_pts):
        if k > 0:
            state = em_step(state, dt, -(state @ lin_a[k - 1].T) + off_b[k - 1], em_noise(seed, k, slots, index, fac))
        visited[k] = state
        if k in gathers:
            state = state[gathers[k]]
    return visited, state
