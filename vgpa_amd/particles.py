"""
ParticleFilterResult: one problem's record of the guided particle filter (vgpa_particle_filter).

The posterior process is the proposal.  Its draws are weighted against the model SDE and the data as in weights.PathWeights, but the
weights are taken in observation by observation, and the cloud of n particles is resampled (systematic resampling) whenever its effective
sample size drops below ess_fraction n.  Resampling preserves the mean weight, so log_evidence() is the formula of PathWeights: with
ess_fraction = 0 the record holds exactly the weights of importance_weights(); with resampling the estimate stays unbiased and its variance
grows linearly, not exponentially, with the number of observations.  Resampling couples the particles of a problem: from the first
resampling on, particle i depends on n (the prefix property of sample_paths ends there).

PathStatistics: one problem's record of vgpa_particle_statistics -- the same filter, every particle carrying along its
lineage the complete-data sufficient statistics of the Euler-discretised model,
    Q_j = sum_k r_j^2 / dt,  G_j = sum_k phi_j r_j,  H_j = sum_k dt phi_j^2,  r = x_k - x_{k-1} - dt f_theta(x_{k-1}),  phi_j = df_j / dtheta_a(j).
The complete-data log-likelihood at theta + delta, Sigma' is -1/2 sum_j [(Q_j - 2 delta_a(j) G_j + delta_a(j)^2 H_j) / Sigma'_jj +
n_steps log(2 pi Sigma'_jj dt)]: quadratic in delta with a diagonal Hessian.  By Fisher's identity the weighted mean of G / Sigma over the
smoothing distribution is the score of log p(y | theta, Sigma), and score / information is the exact EM step in theta.
There is no Sigma step: the paths are imputed at the Sigma in force, their quadratic variation is Sigma T as dt -> 0 whatever the data
say, so Sigma <- E[Q] / n_steps barely moves (0.77 .. 0.79 from Sigma = 0.8 on the fixtures at dt = 0.01).  Q serves the Q-function and as a
diagnostic.

PathEvents: one problem's record of vgpa_particle_events -- the same filter, every particle carrying along its lineage
the records of the event side_j (x_j - level_j) > 0: the largest excursion X, the first grid index T of the event and the number N of grid
indices in it.  Their weighted means and the distribution of T on the grid are reduced on the device: the probability that a component
crossed its level anywhere in the window, the first-passage distribution, the expected occupation time and the expected extreme, from all
n lineages.  The estimator is that of PathStatistics (the final weights on the surviving lineages): exact for the Euler-discretised model
as n grows; in early stretches it rests on the few lineages the genealogy has left there (lineage_ess of SmoothingMoments says how few).

SmoothingMoments: one problem's record of vgpa_particle_moments -- the smoothing mean and second moment on the time grid
under the filter's genealogy.  The final weights are pushed backwards through the ancestors (descendant_weights): the weight of slot a in
the stretch between observations j-1 and j is the total final weight of the slots that descend from it, and
    E[x_k | y] ~ sum_i W^{j(k)}_i x_i(k)
with x_i(k) the state of slot i as the walk arrives at k.  These are the marginals of the forward genealogical smoother: exact in the limit
of many particles for the Euler-discretised model, but early stretches rest on few distinct lineages -- lineage_ess says how few.

SmoothingCovariance: one problem's record of vgpa_particle_covariance -- the same estimate with every cross moment:
    E[x_k x_k^T | y] ~ sum_i W^{j(k)}_i x_i(k) x_i(k)^T,
the full matrix the variational S_t is held against, under the same genealogy and with the same caveat.

SmoothingLagCovariance: one problem's record of vgpa_particle_lag_covariance -- the same estimator at two times,
    E[x_k x_s^T | y] ~ sum_i W_i X_i(k) X_i(s)^T
over the final slots' whole trajectories X_i with the final weights W: the particle counterpart of lagcov.LagCovariance, what the
covariance function K(k, s) of the variational process is held against, under the same genealogy and with the same caveat.

SmoothingMarginals: one problem's record of vgpa_particle_marginals -- the marginal law of x_k[d] | y itself under the
same genealogy, as a histogram over a ladder of levels per component: bin(x) = #{l: levels_l < x}, and the mass of a bin is the sum of
the integer weights Q = the descendants' share of q_i = trunc(W_i 2^62) of the lineages whose state falls into it.  Integer sums do not
depend on any order of addition: the record is exact, the CDF on the ladder non-decreasing by construction.  From it: whether a marginal
is bimodal (modes), its quantiles and bands against m_t +- 1.64 sqrt(S_t), and P(x_k[d] > c | y) along the window (exceedance).

SmoothingPaths: one problem's record of vgpa_particle_paths -- K whole trajectories on the time grid from the same
genealogy, for what is no mean or variance: exceedance and first-passage probabilities, plots of posterior draws, predictive checks.  A
trajectory is the lineage of one final slot; the final slots are drawn from the final weights by systematic resampling (equally weighted
draws) or given by the caller (weighted by their final weights).  The same caveat holds: on collapsing clouds the early stretches of all K
trajectories are one and the same path -- distinct() counts how many different ones each stretch has.

Forecast: one problem's record of vgpa_particle_forecast -- a weighted cloud (the filter's final one, or a given one)
carried past the window under the model SDE: mean and variance on the forecast grid, reduced on the device, a handful of member
trajectories, and the cloud at the end of the horizon, from which the next forecast can go on (cloud=state, log_w=log_w,
index0=grid[-1] when the last step is kept).  The weights do not change: there is nothing to weigh the particles against.

GibbsChain: one problem's record of particle Gibbs with ancestor sampling (vgpa_particle_conditional) -- a Markov chain on
(theta, trajectory) whose invariant law is the joint posterior of the Euler-discretised model.  Each iteration runs the conditional
particle filter from the current trajectory at the current theta, then draws theta given the new trajectory: the drift is f0 + Phi theta
with a diagonal Sigma, so that conditional is Gaussian, component by component, with
    information I_a = sum_k dt sum_{i in a} phi_i^2 / Sigma_ii (+ the prior's precision),
    score       s_a = sum_k sum_{i in a} phi_i r_i / Sigma_ii at the current theta (+ precision (prior mean - theta)),
    theta'_a ~ N(theta_a + s_a / I_a, 1 / I_a)
-- the rows G and H of PathStatistics on the one trajectory (path_rows, theta_conditional).  The chain is exact for the Euler-discretised
model whatever the proposal (A_t, b_t) and for any number of particles >= 2: they decide how fast it mixes, not what it converges to.
"""
import numpy as np

__all__ = ["ParticleFilterResult", "PathStatistics", "PathEvents", "SmoothingMoments", "BackwardSmoothingMoments", "SmoothingCovariance", "SmoothingLagCovariance", "SmoothingMarginals", "gaussian_ladder", "SmoothingPaths", "Forecast", "GibbsChain", "descendant_weights",
           "path_rows", "theta_conditional", "theta_draw"]


def descendant_weights(log_w, ancestors, resampled):
    """(M + 1, n): row M is w / sum w with w = exp(log_w - max log_w); row j < M is row j + 1 where the cloud was carried on at observation
    j (resampled[j] false), else W^j_a = sum of W^{j+1}_i over the slots i with ancestors[j, i] = a, added in increasing i; a slot without
    descendant gets 0.  Every row sums to 1 up to rounding.  Row j weighs the cloud at observation j (the states before its resampling
    decision): with ParticleFilterResult.clouds, W[j] @ clouds[j] is the smoothing mean at that observation."""
    log_w = np.asarray(log_w, dtype=float).ravel()
    anc = np.asarray(ancestors, dtype=np.int64).reshape(-1, log_w.size)
    flags = np.asarray(resampled).astype(bool).ravel()
    if flags.size != anc.shape[0]:
        raise ValueError(" descendant_weights: ancestors and resampled do not belong together.")
    out = np.empty((flags.size + 1, log_w.size))
    out[-1] = _weights_of(log_w)
    for j in range(flags.size - 1, -1, -1):
        out[j] = np.bincount(anc[j], weights=out[j + 1], minlength=log_w.size) if flags[j] else out[j + 1]
    return out


def _weights_of(log_w):
    """w / sum w with w = exp(log_w - max log_w)"""
    w = np.exp(log_w - np.max(log_w))
    return w / np.sum(w)


class _WalkRecord(object):
    """What every record of the filter's walk carries: the final log-weights log_w (n,), and ess and resampled over the problem's
    observations.  A record takes them in its own order (_take_weights first, _take_decisions where its checks have it); the texts carry
    the record's own name."""

    def _take_weights(self, log_w):
        self.log_w = np.asarray(log_w, dtype=float).ravel()
        if self.log_w.size < 1:
            raise ValueError(f" {type(self).__name__}: at least one particle.")

    def _take_decisions(self, ess, resampled, what="ess and resampled", also=False):
        """ess and resampled; ValueError where they differ in length, or where `also` says that something else named in `what` does not fit"""
        self.ess = np.asarray(ess, dtype=float).ravel()
        self.resampled = np.asarray(resampled).astype(bool).ravel()
        if also or self.ess.size != self.resampled.size:
            raise ValueError(f" {type(self).__name__}: {what} do not belong together.")

    def __len__(self):
        return self.log_w.size

    def _normalised(self):
        return _weights_of(self.log_w)

    def log_evidence(self):
        """logsumexp(log_w) - log n: the estimate of log p(y | theta, Sigma), unbiased in the evidence with or without resampling"""
        top = np.max(self.log_w)
        return float(top + np.log(np.sum(np.exp(self.log_w - top))) - np.log(self.log_w.size))


class _Strided(object):
    """A record that keeps every stride-th of n_pts grid indices: the two numbers and their check"""

    def _take_grid(self, stride, n_pts):
        self.stride, self.n_pts = int(stride), int(n_pts)
        if self.stride < 1 or self.n_pts < 1:
            raise ValueError(f" {type(self).__name__}: stride and n_pts must be at least 1.")
        return (self.n_pts - 1) // self.stride + 1


class _KeptGrid(_Strided):
    """... with the kept grid indices 0, stride, 2 stride, ... < n_pts computed on demand and, with obs_t, the stretch between observations
    each of them lies in"""

    @property
    def grid(self):
        """the kept grid indices 0, stride, 2 stride, ..."""
        return np.arange(0, self.n_pts, self.stride)

    def _stretch_on_grid(self):
        """index k belongs to stretch #{observations before k}"""
        return np.searchsorted(self.obs_t, self.grid, side="left")


class ParticleFilterResult(_WalkRecord):
    """log_w (n,): the final unnormalised log-weights; state (n, D): the final particles; over the problem's M_p observations: ess (M_p,),
    resampled (M_p,) bool, and -- history=True, else None -- ancestors (M_p, n): slot i behind observation j came from slot ancestors[j, i]
    of clouds[j] (the identity where the cloud was carried on), clouds (M_p, n, D): the particles at observation j before the resampling
    decision.  The 1-D models drop the last axis of state and clouds."""

    def __init__(self, log_w, state, ess, resampled, ancestors=None, clouds=None) -> None:
        self._take_weights(log_w)
        self.state = np.asarray(state, dtype=float)
        self.ancestors = None if ancestors is None else np.asarray(ancestors, dtype=np.int64)
        self.clouds = None if clouds is None else np.asarray(clouds, dtype=float)
        self._take_decisions(ess, resampled, "log_w, state, ess and resampled", self.state.shape[0] != self.log_w.size)
        if self.ancestors is not None and self.ancestors.shape != (self.ess.size, self.log_w.size):
            raise ValueError(" ParticleFilterResult: ancestors must be (observations, particles).")

    def final_ess(self):
        """(sum w)^2 / sum w^2 of the final weights, between 1 and n"""
        w = np.exp(self.log_w - np.max(self.log_w))
        return float(np.sum(w) ** 2 / np.sum(w * w))

    def mean(self, values):
        """The self-normalised weighted mean over the leading axis of values (n, ...), e.g. of state (the filtering mean at the last grid
        point) or of lineages()."""
        return np.tensordot(self._normalised(), np.asarray(values, dtype=float), axes=(0, 0))

    def lineages(self):
        """(n, M_p, D) ((n, M_p) for the 1-D models): final slot i traced back through `ancestors`, its point at observation j taken from
        clouds[j] -- with log_w, weighted smoothing trajectories at the observation times.  Needs the histories (history=True)."""
        if self.ancestors is None or self.clouds is None:
            raise ValueError(" ParticleFilterResult: lineages() needs the histories (particle_filter(..., history=True)).")
        n, m = self.log_w.size, self.ess.size
        out = np.empty((n, m) + self.clouds.shape[2:])
        slot = np.arange(n)
        for j in range(m - 1, -1, -1):
            slot = self.ancestors[j, slot]
            out[:, j] = self.clouds[j, slot]
        return out

    def smoothing_weights(self):
        """(M_p + 1, n): descendant_weights of the record -- row j weighs clouds[j], so that the smoothing mean at observation j is
        smoothing_weights()[j] @ clouds[j], equal to mean(lineages())[j] up to rounding without tracing a lineage.  Needs the ancestors."""
        if self.ancestors is None:
            raise ValueError(" ParticleFilterResult: smoothing_weights() needs the histories (particle_filter(..., history=True)).")
        return descendant_weights(self.log_w, self.ancestors, self.resampled)


class PathStatistics(_WalkRecord):
    """log_w (n,): the final unnormalised log-weights; mean (3, D): the self-normalised weighted mean of the rows (Q, G, H); rows
    (n, 3, D): the rows themselves, or None; ess, resampled over the problem's observations; dt, n_steps = Np - 1 and model ("OU", "DW",
    "L63", "L96") say how the rows were made.  sigma_diag below: the diagonal of Sigma, (D,) or a scalar."""

    def __init__(self, log_w, mean, dt, n_steps, model, ess=(), resampled=(), rows=None) -> None:
        self._take_weights(log_w)
        self.mean = np.asarray(mean, dtype=float)
        if self.mean.ndim != 2 or self.mean.shape[0] != 3:
            raise ValueError(" PathStatistics: mean must be (3, D).")
        if model not in ("OU", "DW", "L63", "L96"):
            raise ValueError(f" PathStatistics: unknown model -> {model}")
        if model == "L63" and self.mean.shape[1] != 3:
            raise ValueError(" PathStatistics: Lorenz-63 has three components.")
        self.dt, self.n_steps, self.model = float(dt), int(n_steps), model
        self.rows = None if rows is None else np.asarray(rows, dtype=float)
        if self.rows is not None and self.rows.shape != (self.log_w.size,) + self.mean.shape:
            raise ValueError(" PathStatistics: rows must be (particles, 3, D).")
        self._take_decisions(ess, resampled)

    @property
    def dim_d(self):
        return self.mean.shape[1]

    @property
    def n_theta(self):
        return 3 if self.model == "L63" else 1

    def expected(self):
        """(E[Q], E[G], E[H]), each (D,)"""
        return self.mean[0].copy(), self.mean[1].copy(), self.mean[2].copy()

    def _over_sigma(self, row, sigma_diag):
        v = row / np.broadcast_to(np.asarray(sigma_diag, dtype=float).ravel(), row.shape)
        return v.copy() if self.model == "L63" else np.array([v.sum()])

    def score(self, sigma_diag):
        """(n_theta,): sum_{j in a} E[G_j] / Sigma_jj, the estimate of grad_theta log p(y | theta, Sigma) of the Euler-discretised model"""
        return self._over_sigma(self.mean[1], sigma_diag)

    def information(self, sigma_diag):
        """(n_theta,): sum_{j in a} E[H_j] / Sigma_jj, minus the (diagonal) Hessian of the Q-function in theta"""
        return self._over_sigma(self.mean[2], sigma_diag)

    def theta_step(self, sigma_diag):
        """(n_theta,): score / information; theta + step is the exact EM update (for Lorenz-63 it does not depend on Sigma)"""
        return self.score(sigma_diag) / self.information(sigma_diag)

    def expected_loglik(self, theta_new, sigma_diag_new, theta_old):
        """The EM Q-function at (theta_new, Sigma_new) from the statistics taken at theta_old:
        -1/2 sum_j [(E[Q_j] - 2 delta_a E[G_j] + delta_a^2 E[H_j]) / Sigma'_jj + n_steps log(2 pi Sigma'_jj dt)], delta = theta_new - theta_old"""
        delta = np.atleast_1d(np.asarray(theta_new, dtype=float)) - np.atleast_1d(np.asarray(theta_old, dtype=float))
        delta = np.broadcast_to(delta, (self.dim_d,)) if self.model != "L63" else delta.reshape(3)
        sg = np.broadcast_to(np.asarray(sigma_diag_new, dtype=float).ravel(), (self.dim_d,))
        q, g, h = self.mean
        return float(-0.5 * np.sum((q - 2.0 * delta * g + delta * delta * h) / sg + self.n_steps * np.log(2.0 * np.pi * sg * self.dt)))


class PathEvents(_WalkRecord, _Strided):
    """log_w (n,): the final unnormalised log-weights; mean (3, D): the self-normalised weighted mean of the rows (X, T, N); cdf (n_keep, D):
    the weighted share of lineages whose component j has been beyond its level at or before the grid indices 0, stride, ...; levels (D,),
    side (D,) of +1 / -1: the event of component j is side_j (x_j - levels_j) > 0; n_pts = Np and dt: the grid; rows (n, 3, D): the rows
    themselves, or None; ess, resampled over the problem's observations.  T = n_pts in a row says: never in the window."""

    def __init__(self, log_w, mean, cdf, levels, side, stride, n_pts, dt, ess=(), resampled=(), rows=None) -> None:
        self._take_weights(log_w)
        self.mean = np.asarray(mean, dtype=float)
        if self.mean.ndim != 2 or self.mean.shape[0] != 3:
            raise ValueError(" PathEvents: mean must be (3, D).")
        d = self.mean.shape[1]
        self.dt = float(dt)
        self.grid = np.arange(self._take_grid(stride, n_pts)) * self.stride
        self.cdf = np.asarray(cdf, dtype=float)
        if self.cdf.shape != (self.grid.size, d):
            raise ValueError(" PathEvents: cdf must be (n_keep, D).")
        self.levels = np.broadcast_to(np.asarray(levels, dtype=float).ravel(), (d,)).copy()
        self.side = np.broadcast_to(np.asarray(side).ravel(), (d,)).astype(int)
        if not np.all(np.abs(self.side) == 1):
            raise ValueError(" PathEvents: side must be +1 or -1.")
        self.rows = None if rows is None else np.asarray(rows, dtype=float)
        if self.rows is not None and self.rows.shape != (self.log_w.size,) + self.mean.shape:
            raise ValueError(" PathEvents: rows must be (particles, 3, D).")
        self._take_decisions(ess, resampled)

    @property
    def dim_d(self):
        return self.mean.shape[1]

    def weights(self):
        """(n,): w / sum w with w = exp(log_w - max log_w)"""
        return self._normalised()

    @property
    def prob_crossed(self):
        """(D,): the probability that component j was beyond its level at some grid index of the window: the last row of cdf when the kept
        grid ends at the last grid index, else the weighted share of the rows with T < n_pts (per_particle=True)"""
        if (self.n_pts - 1) % self.stride == 0:
            return self.cdf[-1].copy()
        if self.rows is None:
            raise ValueError(" PathEvents: the kept grid ends before the last grid index; prob_crossed then needs the rows (per_particle=True).")
        return np.tensordot(self.weights(), (self.rows[:, 1] < self.n_pts).astype(float), axes=(0, 0))

    def first_passage_cdf(self):
        """(grid (n_keep,), cdf (n_keep, D)): P(T_j <= k | y) at the kept grid indices k; multiply grid by dt for times"""
        return self.grid.copy(), self.cdf.copy()

    def first_passage_quantile(self, q):
        """(D,): the smallest kept grid index k with P(T_j <= k | y) >= q, NaN where the distribution does not reach q in the window"""
        if not 0.0 < float(q) <= 1.0:
            raise ValueError(" PathEvents: q must lie in (0, 1].")
        hit = self.cdf >= float(q)
        first = np.argmax(hit, axis=0)
        return np.where(hit.any(axis=0), self.grid[first].astype(float), np.nan)

    @property
    def occupation_time(self):
        """(D,): dt E[N_j], the expected time component j spent beyond its level (in grid steps of length dt, the start included)"""
        return self.dt * self.mean[2]

    @property
    def mean_extreme(self):
        """(D,): levels + side E[X], in the caller's units: the expected maximum of x_j over the window for side +1, its minimum for -1"""
        return self.levels + self.side * self.mean[0]

    def extreme_quantile(self, q):
        """(D,): levels + side X_q with X_q the weighted q-quantile of the rows' X (the smallest X whose cumulated weight reaches q): for
        side +1 the q-quantile of the window's maximum of x_j, for side -1 the (1 - q)-quantile of its minimum.  Needs the rows."""
        if self.rows is None:
            raise ValueError(" PathEvents: extreme_quantile needs the rows (per_particle=True).")
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(" PathEvents: q must lie in [0, 1].")
        w, out = self.weights(), np.empty(self.dim_d)
        for j in range(self.dim_d):
            order = np.argsort(self.rows[:, 0, j], kind="stable")
            cum = np.cumsum(w[order])
            out[j] = self.rows[order[min(int(np.searchsorted(cum, float(q) * cum[-1], side="left")), order.size - 1)], 0, j]
        return self.levels + self.side * out


class _GenealogySums(_WalkRecord, _KeptGrid):
    """The sums on the kept grid under the filter's genealogy: with them obs_t and lineage_ess (M_p + 1,), one entry per stretch"""

    def _take_stretches(self, obs_t, lineage_ess, ess, resampled):
        self.obs_t = np.asarray(obs_t, dtype=np.int64).ravel()
        self.lineage_ess = np.asarray(lineage_ess, dtype=float).ravel()
        self._take_decisions(ess, resampled, "obs_t, lineage_ess, ess and resampled", self.lineage_ess.size != self.obs_t.size + 1)

    def lineage_ess_on_grid(self):
        """lineage_ess of the stretch each kept grid index lies in: index k belongs to stretch #{observations before k}"""
        return self.lineage_ess[self._stretch_on_grid()]


class SmoothingMoments(_GenealogySums):
    """log_w (n,): the final unnormalised log-weights; moments (n_keep, 2, D): sum_i W_i x_i(k) and sum_i W_i x_i(k)^2 at the grid indices
    k = 0, stride, 2 stride, ... < n_pts; obs_t: the problem's own observation indices; lineage_ess (M_p + 1,): 1 / sum W^2 of every stretch;
    ess, resampled over the problem's observations.  single_dim: a 1-D model, the last axis of mean / second / var / std is dropped."""

    def __init__(self, log_w, moments, stride, n_pts, obs_t, lineage_ess, ess=(), resampled=(), single_dim=False) -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        self.moments = np.asarray(moments, dtype=float)
        if self.moments.ndim != 3 or self.moments.shape[:2] != (n_keep, 2):
            raise ValueError(" SmoothingMoments: moments must be (n_keep, 2, D).")
        self._take_stretches(obs_t, lineage_ess, ess, resampled)
        self.single_dim = bool(single_dim)

    def _shape(self, a):
        return a[..., 0] if self.single_dim else a

    @property
    def mean(self):
        """E[x_k | y] on the grid"""
        return self._shape(self.moments[:, 0].copy())

    @property
    def second(self):
        """E[x_k^2 | y], component by component"""
        return self._shape(self.moments[:, 1].copy())

    @property
    def var(self):
        """second - mean^2, as it comes: where a stretch rests on one lineage the difference is rounding noise of either sign"""
        return self._shape(self.moments[:, 1] - self.moments[:, 0] ** 2)

    @property
    def std(self):
        return np.sqrt(np.maximum(self.var, 0.0))


class BackwardSmoothingMoments(_WalkRecord, _KeptGrid):
    """One problem's record of vgpa_particle_backward_moments: SmoothingMoments' sums under the weights of the marginal
    backward smoother.  log_w (n,): the final unnormalised log-weights; moments (n_keep, 2, D): sum_i W_i x_i(k) and sum_i W_i x_i(k)^2 at the
    grid indices k = 0, stride, 2 stride, ... < n_pts; obs_t: the problem's own observation indices; smoothing_ess (M_p + 1,): 1 / sum W^2 of
    every stretch; weights (M_p + 1, n): W^j_i, every row summing to 1, or None; ess, resampled over the problem's observations.  A stretch's
    weights come from all n particles of the cloud behind it, so early stretches do not rest on the one lineage the genealogy leaves there
    -- where the clouds overlap.  Where the particles of a cloud lie many transition widths apart (high D, few observations) the table is
    the genealogy's and so is every number here.  single_dim: a 1-D model, the last axis of mean / second / var / std is dropped."""

    def __init__(self, log_w, moments, stride, n_pts, obs_t, smoothing_ess, weights=None, ess=(), resampled=(), single_dim=False) -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        self.moments = np.asarray(moments, dtype=float)
        if self.moments.ndim != 3 or self.moments.shape[:2] != (n_keep, 2):
            raise ValueError(" BackwardSmoothingMoments: moments must be (n_keep, 2, D).")
        self.obs_t = np.asarray(obs_t, dtype=np.int64).ravel()
        self.smoothing_ess = np.asarray(smoothing_ess, dtype=float).ravel()
        self.weights = None if weights is None else np.asarray(weights, dtype=float)
        fits = self.weights is None or self.weights.shape == (self.obs_t.size + 1, self.log_w.size)
        self._take_decisions(ess, resampled, "obs_t, smoothing_ess, weights, ess and resampled", self.smoothing_ess.size != self.obs_t.size + 1 or not fits)
        self.single_dim = bool(single_dim)

    _shape = SmoothingMoments._shape
    mean, second, var, std = SmoothingMoments.mean, SmoothingMoments.second, SmoothingMoments.var, SmoothingMoments.std

    def smoothing_ess_on_grid(self):
        """smoothing_ess of the stretch each kept grid index lies in: index k belongs to stretch #{observations before k}"""
        return self.smoothing_ess[self._stretch_on_grid()]


class SmoothingCovariance(_GenealogySums):
    """log_w (n,): the final unnormalised log-weights; mean (n_keep, D): sum_i W_i x_i(k) and second (n_keep, D, D): sum_i W_i x_i(k) x_i(k)^T
    at the grid indices k = 0, stride, 2 stride, ... < n_pts; obs_t: the problem's own observation indices; lineage_ess (M_p + 1,): 1 / sum W^2
    of every stretch; ess, resampled over the problem's observations.  single_dim: a 1-D model, the component axes of mean / second / cov /
    var / corr are dropped."""

    def __init__(self, log_w, mean, second, stride, n_pts, obs_t, lineage_ess, ess=(), resampled=(), single_dim=False) -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        self._mean, self._second = np.asarray(mean, dtype=float), np.asarray(second, dtype=float)
        if self._mean.ndim != 2 or self._mean.shape[0] != n_keep or self._second.shape != (n_keep, self._mean.shape[1], self._mean.shape[1]):
            raise ValueError(" SmoothingCovariance: mean must be (n_keep, D) and second (n_keep, D, D).")
        self._take_stretches(obs_t, lineage_ess, ess, resampled)
        self.single_dim = bool(single_dim)

    def _vec(self, a):
        return a[..., 0] if self.single_dim else a

    def _mat(self, a):
        return a[..., 0, 0] if self.single_dim else a

    @property
    def mean(self):
        """E[x_k | y] on the grid"""
        return self._vec(self._mean.copy())

    @property
    def second(self):
        """E[x_k x_k^T | y], the raw second-moment matrices"""
        return self._mat(self._second.copy())

    def _cov(self):
        return self._second - self._mean[:, :, None] * self._mean[:, None, :]

    @property
    def cov(self):
        """second - mean mean^T, as it comes and not clipped: where a stretch rests on one lineage the difference is rounding noise, and
        the matrix need not be positive semi-definite"""
        return self._mat(self._cov())

    @property
    def var(self):
        """the diagonal of cov"""
        return self._vec(np.diagonal(self._cov(), axis1=1, axis2=2).copy())

    @property
    def corr(self):
        """cov_ab / sqrt(cov_aa cov_bb); nan where a variance is not positive"""
        c = self._cov()
        v = np.diagonal(c, axis1=1, axis2=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.sqrt(np.where(v > 0.0, v, np.nan))
            return self._mat(c / (s[:, :, None] * s[:, None, :]))

    def gaussian(self, k):
        """(mean, cov) at the grid index k, which must be a kept one (ValueError otherwise).  At k = n_pts - 1 no observation lies behind k:
        that is the filtering Gaussian a following window takes as its m0, S0."""
        k = int(k)
        if k < 0 or k >= self.n_pts or k % self.stride:
            raise ValueError(f" SmoothingCovariance: grid index {k} is not kept (stride {self.stride}, n_pts {self.n_pts}).")
        i = k // self.stride
        return self._vec(self._mean[i].copy()), self._mat(self._cov()[i])


class SmoothingLagCovariance(_GenealogySums):
    """The two-time moments of the smoothing law (vgpa_particle_lag_covariance), the particle counterpart of
    lagcov.LagCovariance -- cov, corr, increment_var and joint take the same arguments and mean the same --: log_w (n,): the final
    unnormalised log-weights; mean (n_keep, D): sum_i W_i x_i(k); cross (n_anchor, n_keep, D, D): block [q, j] is
    sum_i W_i x_i(grid[j]) x_i(anchors[q])^T, filled on both sides of the anchor; anchors (n_anchor,): strictly increasing kept grid
    indices; obs_t, lineage_ess, ess, resampled as SmoothingCovariance.  single_dim: a 1-D model, the component axes of every result are
    dropped.  Nothing is clipped: where a stretch rests on one lineage a variance is rounding noise of either sign and stays so."""

    def __init__(self, log_w, mean, cross, anchors, stride, n_pts, obs_t, lineage_ess, ess=(), resampled=(), single_dim=False) -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        self._mean, self._cross = np.asarray(mean, dtype=float), np.asarray(cross, dtype=float)
        self.anchors = np.asarray(anchors, dtype=np.int64).ravel()
        if self._mean.ndim != 2 or self._mean.shape[0] != n_keep or self._cross.shape != (self.anchors.size, n_keep) + 2 * (self._mean.shape[1],):
            raise ValueError(" SmoothingLagCovariance: mean must be (n_keep, D) and cross (n_anchor, n_keep, D, D).")
        if self.anchors.size < 1 or np.any(np.diff(self.anchors) <= 0) or self.anchors[0] < 0 or self.anchors[-1] >= self.n_pts or np.any(self.anchors % self.stride):
            raise ValueError(" SmoothingLagCovariance: anchors must be strictly increasing kept grid indices.")
        self._take_stretches(obs_t, lineage_ess, ess, resampled)
        self.single_dim = bool(single_dim)
        self._anchor_at = {int(s): q for q, s in enumerate(self.anchors)}

    def _vec(self, a):
        return a[..., 0] if self.single_dim else a

    def _mat(self, a):
        return a[..., 0, 0] if self.single_dim else a

    @property
    def mean(self):
        """E[x_k | y] on the kept grid"""
        return self._vec(self._mean.copy())

    @property
    def cross(self):
        """E[x_k x_s^T | y], the raw cross moments of every anchor s"""
        return self._mat(self._cross.copy())

    def _row(self, k):
        k = int(k)
        if k < 0 or k >= self.n_pts or k % self.stride:
            raise KeyError(f"grid index {k} is not on the kept grid (stride {self.stride}, n_pts {self.n_pts})")
        return k // self.stride

    def _block(self, k, s):
        """cross - mean mean^T at kept index k and anchor s, (D, D)"""
        j, i = self._row(k), self._row(s)
        return self._cross[self._anchor_at[int(s)], j] - self._mean[j][:, None] * self._mean[i][None, :]

    def _cov(self, k, s):
        k, s = int(k), int(s)
        if s in self._anchor_at:
            return self._block(k, s)
        if k in self._anchor_at:
            return self._block(s, k).T
        raise KeyError(f"neither {k} nor {s} is an anchor (anchors: {self.anchors.tolist()})")

    def cov(self, k, s):
        """Cov[x_k, x_s | y] = cross - mean_k mean_s^T, (D, D), as it comes: the block of anchor s at the kept index k, or the transpose of
        the block of anchor k at the kept index s.  KeyError where neither index is an anchor or the other one is not kept."""
        return self._mat(self._cov(k, s))

    def _marginal(self, k, st=None):
        if st is None:
            return self._cov(k, k)
        st = np.asarray(st, dtype=float)
        if st.ndim == 1:
            st = st[:, None, None]
        return st[self._row(k)]

    def marginal(self, k, st=None):
        """Cov[x_k | y], (D, D): from st (n_keep, D, D), the marginal covariances on the kept grid (SmoothingCovariance.cov), or -- st=None
        -- from the row k of anchor k"""
        return self._mat(self._marginal(k, st))

    def _corr(self, k, s, st=None):
        vk, vs = np.diagonal(self._marginal(k, st)), np.diagonal(self._marginal(s, st))
        with np.errstate(invalid="ignore", divide="ignore"):
            dk, ds = np.sqrt(np.where(vk > 0.0, vk, np.nan)), np.sqrt(np.where(vs > 0.0, vs, np.nan))
            return self._cov(k, s) / (dk[:, None] * ds[None, :])

    def corr(self, k, s, st=None):
        """Corr[x_k,a, x_s,b] = cov_ab / sqrt(Var x_k,a Var x_s,b), (D, D); the marginals as in marginal(); nan where a variance is not
        positive"""
        return self._mat(self._corr(k, s, st))

    def increment_var(self, k, s, st=None):
        """Cov[x_k - x_s | y] = S_k + S_s - C - C^T with C = cov(k, s), (D, D), not clipped"""
        c = self._cov(k, s)
        return self._mat(self._marginal(k, st) + self._marginal(s, st) - c - c.T)

    def autocorrelation(self, s, var=None):
        """Corr[x_k,a, x_s,a] of anchor s at every kept grid index k, (n_keep, D).  var (n_keep, D): the marginal variances on the kept
        grid (SmoothingMoments.var, SmoothingCovariance.var); None: they are known at the anchors alone, and the other rows are nan."""
        q = self._anchor_at.get(int(s))
        if q is None:
            raise KeyError(f"{int(s)} is not an anchor (anchors: {self.anchors.tolist()})")
        i = self._row(s)
        c = np.diagonal(self._cross[q], axis1=1, axis2=2) - self._mean * self._mean[i][None, :]
        if var is None:
            v = np.full(self._mean.shape, np.nan)
            for a in self.anchors:
                v[self._row(a)] = np.diagonal(self._cov(a, a))
        else:
            v = np.asarray(var, dtype=float).reshape(self._mean.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.sqrt(np.where(v > 0.0, v, np.nan))
            return self._vec(c / (d * d[i][None, :]))

    def joint(self):
        """(mean (n_anchor D,), covariance (n_anchor D, n_anchor D)) of the stacked anchor states (x_{s_1}, ..., x_{s_n}) | y: block (i, j)
        of the covariance is cov(s_i, s_j), taken from the anchor rows of cross for j <= i and transposed above the diagonal; the diagonal
        blocks are symmetrised (their two triangles are two roundings of the same sum)."""
        n, d = self.anchors.size, self._mean.shape[1]
        m = np.concatenate([self._mean[self._row(s)] for s in self.anchors])
        out = np.empty((n * d, n * d))
        for i, si in enumerate(self.anchors):
            for j, sj in enumerate(self.anchors[:i + 1]):
                c = self._cov(si, sj)
                if j == i:
                    c = 0.5 * (c + c.T)
                out[i * d:(i + 1) * d, j * d:(j + 1) * d] = c
                out[j * d:(j + 1) * d, i * d:(i + 1) * d] = c.T
        return m, out


def gaussian_ladder(mt, st, n_levels=31, width=4.0):
    """(D, n_levels): per component a uniform ladder from min_k (m - width sqrt(S)) to max_k (m + width sqrt(S)) of a Gaussian posterior on the
    grid.  mt (Np, D) or (Np,): the means; st (Np, D, D), (Np, D) or (Np,): the covariance matrices or the variances."""
    m = np.asarray(mt, dtype=float)
    m = m.reshape(m.shape[0], -1)
    v = np.asarray(st, dtype=float)
    v = np.diagonal(v, axis1=1, axis2=2) if v.ndim == 3 else v.reshape(v.shape[0], -1)
    n_levels, width = int(n_levels), float(width)
    if v.shape != m.shape or n_levels < 1 or not width > 0.0:
        raise ValueError(" gaussian_ladder: mt (Np, D) and st (Np, D, D) or (Np, D) must belong together, n_levels >= 1, width > 0.")
    sd = np.sqrt(np.maximum(v, 0.0))
    lo, hi = np.min(m - width * sd, axis=0), np.max(m + width * sd, axis=0)
    if n_levels == 1:
        return (0.5 * (lo + hi))[:, None]
    out = lo[:, None] + (hi - lo)[:, None] * (np.arange(n_levels) / (n_levels - 1.0))[None, :]
    out[:, -1] = hi      # (the ends as computed: the ladder covers m +- width sqrt(S) to the bit)
    return out


def posterior_ladders(ctx, n_levels=31, width=4.0):
    """(B, D, n_levels): gaussian_ladder of every problem's Gaussian posterior (m_t, S_t) as the context `ctx` holds it from its last
    evaluation of F (fetched; the cached state stays as it is)"""
    mt = np.asarray(ctx.fetch("mt"), dtype=float).reshape(ctx.B, ctx.Np, ctx.D)
    st = np.asarray(ctx.fetch("st"), dtype=float).reshape(ctx.B, ctx.Np, ctx.D, ctx.D)
    return np.stack([gaussian_ladder(mt[p], st[p], n_levels, width) for p in range(ctx.B)])


class SmoothingMarginals(_GenealogySums):
    """log_w (n,): the final unnormalised log-weights; levels (D, L): per component a strictly increasing ladder; mass (n_keep, D, L + 1)
    uint64: the integer weight of the lineages whose component d lies in bin b = #{l: levels[d, l] < x} at the grid indices k = 0, stride,
    ... < n_pts; q_final (n,) uint64: trunc(W 2^62) of the final weights; obs_t, lineage_ess, ess, resampled as in SmoothingMoments.
    single_dim: a 1-D model, the component axis of cdf / hist / exceedance / quantile / band / modes is dropped."""

    def __init__(self, log_w, levels, mass, q_final, stride, n_pts, obs_t, lineage_ess, ess=(), resampled=(), single_dim=False) -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        self.levels = np.asarray(levels, dtype=float)
        if self.levels.ndim != 2 or self.levels.shape[1] < 1 or not np.all(self.levels[:, 1:] > self.levels[:, :-1]):
            raise ValueError(" SmoothingMarginals: levels must be (D, L), strictly increasing along L.")
        self.mass = np.asarray(mass)
        if self.mass.dtype != np.uint64 or self.mass.shape != (n_keep,) + (self.levels.shape[0], self.levels.shape[1] + 1):
            raise ValueError(" SmoothingMarginals: mass must be uint64 (n_keep, D, L + 1).")
        self.q_final = np.asarray(q_final, dtype=np.uint64).ravel()
        if self.q_final.size != self.log_w.size:
            raise ValueError(" SmoothingMarginals: q_final must hold one weight per particle.")
        self._take_stretches(obs_t, lineage_ess, ess, resampled)
        self.single_dim = bool(single_dim)

    def _shape(self, a, axis=1):
        return np.take(a, 0, axis=axis) if self.single_dim else a

    def total(self):
        """(n_keep, D) uint64: the sum over the bins, in integer arithmetic -- the same for every component and every kept index of a stretch"""
        return self._shape(self.mass.sum(axis=2, dtype=np.uint64))

    def _cdf(self):
        cum = np.cumsum(self.mass, axis=2, dtype=np.uint64)
        return cum[:, :, :-1].astype(float) / cum[:, :, -1:].astype(float)

    def cdf(self):
        """(n_keep, D, L): P(x_k[d] <= levels[d, l] | y), the exact integer prefix sums over the total: non-decreasing in l, within [0, 1]"""
        return self._shape(self._cdf())

    def hist(self):
        """(n_keep, D, L + 1): the probability of every bin"""
        return self._shape(self.mass.astype(float) / self.mass.sum(axis=2, dtype=np.uint64).astype(float)[:, :, None])

    def exceedance(self, level_index):
        """(n_keep, D): P(x_k[d] > levels[d, level_index] | y) = 1 - cdf"""
        return self._shape(1.0 - self._cdf()[:, :, range(self.levels.shape[1])[int(level_index)]])

    def _quantile(self, q):
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(" SmoothingMarginals: q must lie in [0, 1].")
        cdf, lev = self._cdf(), self.levels
        n_levels = lev.shape[1]
        out = np.empty(cdf.shape[:2])
        for d in range(lev.shape[0]):
            for k in range(cdf.shape[0]):
                c = cdf[k, d]
                hi = int(np.searchsorted(c, q, side="left"))      # the first level whose cdf reaches q
                if hi == 0:
                    out[k, d] = lev[d, 0] if q == c[0] else -np.inf
                elif hi == n_levels:
                    out[k, d] = np.inf
                elif c[hi] == q:
                    out[k, d] = lev[d, hi]
                else:
                    out[k, d] = lev[d, hi - 1] + (lev[d, hi] - lev[d, hi - 1]) * (q - c[hi - 1]) / (c[hi] - c[hi - 1])
        return out

    def quantile(self, q):
        """(n_keep, D): the q-quantile of every marginal, linear inside the pair of levels that brackets it; -inf / +inf where q lies in the
        open bin below the first / above the last level"""
        return self._shape(self._quantile(q))

    def band(self, lo=0.05, hi=0.95):
        """(quantile(lo), quantile(hi)): e.g. the 5 % and 95 % quantiles, to hold against m_t -+ 1.64 sqrt(S_t)"""
        if not float(lo) <= float(hi):
            raise ValueError(" SmoothingMarginals: lo must not exceed hi.")
        return self.quantile(lo), self.quantile(hi)

    def modes(self, k):
        """(D,) int: the number of interior local maxima of the bin density mass / bin width at the grid index k, which must be a kept one
        (ValueError otherwise): a maximal run of equal densities counts once, where it is higher than both its neighbours; the two open end
        bins have no width and count as density 0.  2 or more: the marginal is multimodal on this ladder."""
        k = int(k)
        if k < 0 or k >= self.n_pts or k % self.stride:
            raise ValueError(f" SmoothingMarginals: grid index {k} is not kept (stride {self.stride}, n_pts {self.n_pts}).")
        dens = self.mass[k // self.stride, :, 1:-1].astype(float) / np.diff(self.levels, axis=1)
        out = np.zeros(self.levels.shape[0], dtype=int)
        for d in range(out.size):
            row = np.concatenate(([0.0], dens[d], [0.0]))
            row = row[np.concatenate(([True], row[1:] != row[:-1]))]      # runs of equal densities: one entry each
            out[d] = int(np.sum((row[1:-1] > row[:-2]) & (row[1:-1] > row[2:])))
        return out[0] if self.single_dim else out


class SmoothingPaths(_WalkRecord, _KeptGrid):
    """log_w (n,): the filter's final unnormalised log-weights; paths (K, n_keep, D): the trajectories at the grid indices k = 0, stride,
    2 stride, ... < n_pts; slots (M_p + 1, K): the slot trajectory m sat in during stretch j (row M_p: its final slot); obs_t: the problem's
    own observation indices; ess, resampled over them.  drawn: the final slots were drawn from the final weights, the trajectories are
    equally weighted; else they are the caller's, and mean() / var() take weights.  single_dim: a 1-D model, the last axis of paths is
    dropped.

    The trajectories are lineages of one genealogy: where the clouds collapsed, all K of them share their early stretches, and a sample
    mean over them has there the variance of a single draw.  distinct() says how many different paths each stretch holds.

    method: how the table `slots` was made.  "genealogy" (vgpa_particle_paths): row j is the ancestor of row j + 1.  "backward"
    (vgpa_particle_backward_paths): at every observation where the cloud was resampled, row j is drawn anew among all
    n slots, in proportion to filter weight times model transition density to the trajectory's next state, so the early stretches do
    not collapse onto the surviving lineages and hold more distinct paths.  What backward simulation does not change: the filter, the
    final slots, the weights of the trajectories, and the stretches themselves -- between two observations a trajectory is still its
    slot's own path, and at a resampled observation it jumps from the cloud's particle to the one its successor was copied from, so
    distinct() is bounded by the distinct slots chosen, never by more than n."""

    def __init__(self, log_w, paths, slots, stride, n_pts, obs_t, ess=(), resampled=(), drawn=True, single_dim=False, method="genealogy") -> None:
        self._take_weights(log_w)
        n_keep = self._take_grid(stride, n_pts)
        full = np.asarray(paths, dtype=float)
        if full.ndim != 3 or full.shape[0] < 1 or full.shape[1] != n_keep:
            raise ValueError(" SmoothingPaths: paths must be (K, n_keep, D).")
        self.single_dim = bool(single_dim)
        self.paths = full[..., 0] if self.single_dim else full
        self.obs_t = np.asarray(obs_t, dtype=np.int64).ravel()
        self.slots = np.asarray(slots, dtype=np.int64)
        if self.slots.shape != (self.obs_t.size + 1, full.shape[0]):
            raise ValueError(" SmoothingPaths: slots must be (M + 1, K).")
        if self.slots.min() < 0 or self.slots.max() >= self.log_w.size:
            raise ValueError(" SmoothingPaths: a slot outside [0, n).")
        self._take_decisions(ess, resampled)
        self.drawn = bool(drawn)
        if method not in ("genealogy", "backward"):
            raise ValueError(" SmoothingPaths: method is 'genealogy' or 'backward'.")
        self.method = method

    def __len__(self):      # (K, not n)
        return self.paths.shape[0]

    def _weights(self, weights):
        if weights is None:
            if not self.drawn:
                raise ValueError(" SmoothingPaths: the final slots were given: pass weights= (final_weights() are those of the filter).")
            return np.full(len(self), 1.0 / len(self))
        w = np.asarray(weights, dtype=float).ravel()
        if w.size != len(self) or np.any(w < 0.0) or not np.sum(w) > 0.0:
            raise ValueError(" SmoothingPaths: weights must be K non-negative numbers with a positive sum.")
        return w / np.sum(w)

    def final_weights(self):
        """the filter's normalised final weights of the trajectories' final slots, renormalised over the K trajectories: the weights of
        given final slots that are all different"""
        w = np.exp(self.log_w - np.max(self.log_w))[self.slots[-1]]
        return w / np.sum(w)

    def mean(self, weights=None):
        """the mean over the trajectories on the grid, (n_keep, D): equal weights for drawn final slots, `weights` (K,) for given ones"""
        return np.tensordot(self._weights(weights), self.paths, axes=(0, 0))

    def var(self, weights=None):
        """the variance over the trajectories on the grid, sum w (x - mean)^2"""
        w = self._weights(weights)
        dev = self.paths - np.tensordot(w, self.paths, axes=(0, 0))[None]
        return np.tensordot(w, dev * dev, axes=(0, 0))

    def lag_covariance(self, anchors, context, weights=None):
        """The two-time moments of these trajectories as a SmoothingLagCovariance (Context.path_cross_moments on `context`, a Context of
        batch 1 and this model's D): equal weights for drawn final slots -- backward simulation's draws, which do not suffer the
        genealogy's collapse --, `weights` (K,) for given ones.  lineage_ess of the record is nan: the trajectories are no genealogy's
        sums."""
        anc = np.asarray(anchors, dtype=np.int64).ravel()
        if anc.size < 1 or np.any(anc % self.stride) or anc.min() < 0 or anc.max() >= self.n_pts:
            raise ValueError(" SmoothingPaths: anchors must be kept grid indices.")
        full = self.paths[..., None] if self.single_dim else self.paths
        mean, cross = context.path_cross_moments(full[None], anc // self.stride, weights=self._weights(weights)[None])
        return SmoothingLagCovariance(self.log_w, mean[0], cross[0], anc, self.stride, self.n_pts, self.obs_t, np.full(self.obs_t.size + 1, np.nan),
                                      self.ess, self.resampled, self.single_dim)

    def distinct(self):
        """(M_p + 1,): the number of different slots among the K trajectories in every stretch -- the number of different paths there.
        Non-decreasing in time; 1 where the genealogy has coalesced."""
        return np.array([np.unique(row).size for row in self.slots])

    def distinct_on_grid(self):
        """distinct() of the stretch each kept grid index lies in: index k belongs to stretch #{observations before k}"""
        return self.distinct()[self._stretch_on_grid()]


class Forecast(object):
    """log_w (n,): the unnormalised log-weights of the cloud, unchanged by the forecast; moments (h_keep, 2, D): sum_i W_i x_i and
    sum_i W_i x_i^2 at the steps h = 0, stride, 2 stride, ... <= horizon behind the absolute grid index index0; members (K, h_keep, D): the
    trajectories of the slots `slots` (K,) on the same steps (K may be 0); state (n, D): the cloud at index0 + horizon; t0, dt: the time of
    grid index 0 and the grid's step.  drawn: the slots were drawn from the weights (equally weighted members), else given.  single_dim: a
    1-D model, the last axis of mean / var / members / state is dropped."""

    def __init__(self, log_w, moments, members, slots, state, index0, horizon, stride, dt, t0=0.0, drawn=True, single_dim=False) -> None:
        self.log_w = np.asarray(log_w, dtype=float).ravel()
        if self.log_w.size < 1:
            raise ValueError(" Forecast: at least one particle.")
        self.index0, self.horizon, self.stride = int(index0), int(horizon), int(stride)
        if self.index0 < 0 or self.horizon < 0 or self.stride < 1:
            raise ValueError(" Forecast: index0 and horizon must be at least 0, stride at least 1.")
        h_keep = self.horizon // self.stride + 1
        self.moments = np.asarray(moments, dtype=float)
        if self.moments.ndim != 3 or self.moments.shape[:2] != (h_keep, 2):
            raise ValueError(" Forecast: moments must be (h_keep, 2, D).")
        d = self.moments.shape[2]
        full, cloud = np.asarray(members, dtype=float), np.asarray(state, dtype=float)
        if full.ndim != 3 or full.shape[1:] != (h_keep, d):
            raise ValueError(" Forecast: members must be (K, h_keep, D).")
        if cloud.shape != (self.log_w.size, d):
            raise ValueError(" Forecast: state must be (n, D).")
        self.slots = np.asarray(slots, dtype=np.int64).ravel()
        if self.slots.size != full.shape[0] or (self.slots.size and (self.slots.min() < 0 or self.slots.max() >= self.log_w.size)):
            raise ValueError(" Forecast: slots must be K slots in [0, n).")
        self.single_dim = bool(single_dim)
        self.members = full[..., 0] if self.single_dim else full
        self.state = cloud[..., 0] if self.single_dim else cloud
        self.dt, self.t0, self.drawn = float(dt), float(t0), bool(drawn)

    def __len__(self):
        return self.log_w.size

    @property
    def grid(self):
        """the absolute grid indices of the kept steps: index0, index0 + stride, ..."""
        return self.index0 + np.arange(0, self.horizon + 1, self.stride)

    @property
    def times(self):
        return self.t0 + self.dt * self.grid

    @property
    def mean(self):
        m = self.moments[:, 0].copy()
        return m[..., 0] if self.single_dim else m

    @property
    def var(self):
        """second moment - mean^2, clipped at 0"""
        v = np.maximum(self.moments[:, 1] - self.moments[:, 0] ** 2, 0.0)
        return v[..., 0] if self.single_dim else v


def path_rows(model, theta, path, dt):
    """(3, D): the rows (Q, G, H) of PathStatistics on one trajectory path (Np, D): Q_i = sum_k r_i^2 / dt, G_i = sum_k phi_i r_i,
    H_i = sum_k dt phi_i^2 with r = x_k - x_{k-1} - dt f_theta(x_{k-1}) and phi_i = d f_i / d theta_a(i) at x_{k-1}.  model: "OU", "DW",
    "L63", "L96"."""
    path = np.asarray(path, dtype=float)
    if path.ndim == 1:
        path = path[:, None]
    x, th, dt = path[:-1], np.atleast_1d(np.asarray(theta, dtype=float)).ravel(), float(dt)
    if model == "OU":
        f, phi = -th[0] * x, -x
    elif model == "DW":
        f, phi = 4.0 * x * (th[0] - x * x), 4.0 * x
    elif model == "L63":
        f = np.stack((th[0] * (x[:, 1] - x[:, 0]), (th[1] - x[:, 2]) * x[:, 0] - x[:, 1], x[:, 0] * x[:, 1] - th[2] * x[:, 2]), axis=1)
        phi = np.stack((x[:, 1] - x[:, 0], x[:, 0], -x[:, 2]), axis=1)
    elif model == "L96":
        f = (np.roll(x, -1, axis=1) - np.roll(x, 2, axis=1)) * np.roll(x, 1, axis=1) - x + th[0]
        phi = np.ones_like(x)
    else:
        raise ValueError(f" path_rows: unknown model -> {model}")
    r = path[1:] - x - dt * f
    return np.stack((np.sum(r * r, axis=0) / dt, np.sum(phi * r, axis=0), dt * np.sum(phi * phi, axis=0)))


def theta_conditional(model, theta, path, dt, sigma_diag, prior=None):
    """(mean, precision), each (n_theta,): the Gaussian law of theta given one trajectory of the Euler-discretised model.  prior: None
    (flat) or (mean, precision) per component."""
    th = np.atleast_1d(np.asarray(theta, dtype=float)).ravel()
    _, g, h = path_rows(model, th, path, dt)
    sg = np.broadcast_to(np.asarray(sigma_diag, dtype=float).ravel(), g.shape)
    score, info = (g / sg, h / sg) if model == "L63" else (np.array([np.sum(g / sg)]), np.array([np.sum(h / sg)]))
    if prior is not None:
        pm, pl = (np.broadcast_to(np.asarray(v, dtype=float).ravel(), th.shape) for v in prior)
        score, info = score + pl * (pm - th), info + pl
    return th + score / info, info


def theta_draw(mean, precision, seed, iteration, problem):
    """theta' = mean + z / sqrt(precision), z the standard normals of numpy.random.Generator(PCG64([seed, iteration, problem])): the
    draw depends on the chain's seed, the iteration and the problem's index in its batch alone."""
    rng = np.random.Generator(np.random.PCG64([int(seed) & 0xFFFFFFFFFFFFFFFF, int(iteration), int(problem)]))
    mean = np.asarray(mean, dtype=float)
    return mean + rng.standard_normal(mean.shape) / np.sqrt(np.asarray(precision, dtype=float))


class GibbsChain(object):
    """theta (iters + 1, n_theta): theta before the first and after every iteration; paths (n_kept, Np, D): the trajectories of the kept
    iterations `kept` (n_kept,) (burn <= it, every thin-th); moved (iters,): the share of grid points at which an iteration's trajectory
    differs from its reference -- 0 means the conditional filter returned the reference, the chain did not move; first (Np, D): the
    reference iteration 0 started from.  single_dim: a 1-D model, the last axis of paths / mean / var is dropped.

    Successive trajectories are dependent draws: mean() and var() are ergodic averages, and moved says how fast the chain forgets.
    The `burn` of the methods counts iterations: paths of iterations < burn and the theta rows they produced are left out."""

    def __init__(self, theta, paths, kept, moved, first=None, single_dim=False) -> None:
        self.theta = np.asarray(theta, dtype=float)
        if self.theta.ndim != 2 or self.theta.shape[0] < 1:
            raise ValueError(" GibbsChain: theta must be (iters + 1, n_theta).")
        full = np.asarray(paths, dtype=float)
        self.kept = np.asarray(kept, dtype=np.int64).ravel()
        self.moved = np.asarray(moved, dtype=float).ravel()
        if full.ndim != 3 or full.shape[0] != self.kept.size or self.moved.size != self.theta.shape[0] - 1:
            raise ValueError(" GibbsChain: paths (n_kept, Np, D), kept (n_kept,) and moved (iters,) do not belong together.")
        if self.kept.size and (self.kept.min() < 0 or self.kept.max() >= self.moved.size or np.any(np.diff(self.kept) <= 0)):
            raise ValueError(" GibbsChain: kept must be increasing iterations in [0, iters).")
        self.single_dim = bool(single_dim)
        self.paths = full[..., 0] if self.single_dim else full
        self.first = None if first is None else np.asarray(first, dtype=float)

    def __len__(self):
        return self.moved.size

    def _after(self, burn):
        sel = self.paths[self.kept >= int(burn)]
        if sel.shape[0] < 1:
            raise ValueError(" GibbsChain: no kept trajectory behind the burn-in.")
        return sel

    def mean(self, burn=0):
        """the ergodic mean of the kept trajectories of the iterations >= burn, (Np, D)"""
        return self._after(burn).mean(axis=0)

    def var(self, burn=0):
        """their variance on the grid"""
        return self._after(burn).var(axis=0)

    def theta_mean(self, burn=0):
        """(n_theta,): the mean of theta after the iterations >= burn"""
        return self.theta[1 + int(burn):].mean(axis=0)

    def theta_var(self, burn=0):
        return self.theta[1 + int(burn):].var(axis=0)
