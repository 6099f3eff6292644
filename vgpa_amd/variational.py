"""
VarGP: host-side mirror of src/var_bayes/variational.py (constructor, `initialization`, `free_energy`,
`gradient(x, eval_fun=False)`, `arg_out`) whose arithmetic runs fused on the GPU:

    free_energy(x) -> vgpa_free_energy : fwd sweep -> E_obs -> E_sde terms -> bwd sweep -> F
    gradient(x)    -> vgpa_gradient    : per-grid-point assembly from the state left resident in HBM
    gradient(x, eval_fun=True) -> vgpa_sweep

Like the reference the object is stateful: `gradient(x)` without `eval_fun` uses the state cached by the last
`free_energy` call (SCG relies on that ordering, src/numerics/optim_scg.py:163-167).
"""
import numpy as np
from scipy.interpolate import CubicSpline

from ._lib import Context, per_problem


class VarGP(object):

    def __init__(self, model, m0, s0, fwd_ode, bwd_ode, likelihood, kl0, obs_y, obs_t, device=0, flags=0, batch=1) -> None:
        self.model = model
        self.fwd_ode, self.bwd_ode = fwd_ode, bwd_ode
        self.kl0, self.likelihood = kl0, likelihood
        self.obs_y, self.obs_t = obs_y, obs_t
        self.dt = self.model.time_step
        if self.model.single_dim:
            self.dim_n, self.dim_d = self.model.sample_path.size, 1
        else:
            self.dim_n, self.dim_d = self.model.sample_path.shape
        self.dim_tot = self.dim_n * self.dim_d * self.dim_d
        self.output = {"m0": m0, "s0": s0}
        self.device, self.flags, self.batch = device, flags, int(batch)
        self._ctx = None
        self._ctx_key = None
        self._e0 = None
        self._stale = set()
        method_f = str(getattr(fwd_ode, "method", "")).lower()
        method_b = str(getattr(bwd_ode, "method", "")).lower()
        if method_f != method_b:
            raise ValueError(f" {self.__class__.__name__}: forward ({method_f}) and backward ({method_b})"
                             f" integration methods differ; the fused sweep needs one method.")
        self._method = method_f

    # ------------------------------------------------------------------------------------------
    def _inputs(self):
        """Everything the device context bakes in at creation, read from the objects NOW."""
        single, d = self.model.single_dim, self.dim_d
        m0, s0 = self.output["m0"], self.output["s0"]
        lik = self.likelihood
        sigma = np.array([[self.model.sigma]], dtype=float) if single else np.asarray(self.model.sigma, dtype=float)
        op = getattr(lik, "operator", None)
        return dict(sigma=sigma, theta=np.atleast_1d(np.asarray(self.model.theta, dtype=float)),
                    m0=np.atleast_1d(np.asarray(m0, dtype=float)), s0=np.asarray(s0, dtype=float).reshape(d, d),
                    obs_t=np.asarray(lik.times, dtype=np.int64), obs_y=np.asarray(lik.values, dtype=float),
                    obs_noise=np.asarray(lik.noise, dtype=float).reshape(d, d),
                    # the default operator is the identity: passing None keeps libvgpa_hip on its diagonal path
                    obs_h=None if getattr(lik, "default_operator", False) else np.asarray(op, dtype=float).reshape(d, d))

    @staticmethod
    def _fingerprint(inputs):
        """Identity of the baked-in inputs: exact bytes for small arrays, a 128-bit digest of the whole buffer beyond (a D >= 257
        sigma / s0 / obs_noise is hashed in well under a millisecond -- nothing next to a sweep at that size)."""
        import hashlib
        key = []
        for name in sorted(inputs):
            a = inputs[name]
            if a is None:
                key.append((name, None))
            elif a.size <= 1 << 16:
                key.append((name, a.shape, a.tobytes()))
            else:
                key.append((name, a.shape, hashlib.blake2b(np.ascontiguousarray(a).data, digest_size=16).digest()))
        return tuple(key)

    def invalidate(self):
        """Drops the device context (and the state cached in it); the next call rebuilds it from the current
        model / likelihood / prior values."""
        if self._ctx is not None:
            self._ctx.close()
        self._ctx, self._ctx_key, self._stale = None, None, set()

    def _context(self):
        # theta, sigma, the observation noise and (m0, s0) are settable on the reference's objects
        # (stochastic_process.py / likelihood.py setters): a context built from older values must not be reused.
        inputs = self._inputs()
        key = self._fingerprint(inputs)
        if self._ctx is not None and key != self._ctx_key:
            self.invalidate()
        # E0 depends on the prior (kl0.mu0 / kl0.tau0 are plain attributes; the reference evaluates kl0 on every
        # free_energy call, variational.py:185): handed to the context per call, never baked in
        prior = tuple(np.asarray(getattr(self.kl0, k, 0.0), dtype=float).tobytes() for k in ("mu0", "tau0"))
        if self._e0 is None or self._e0[0] != (prior, key):
            self._e0 = ((prior, key), float(np.asarray(self.kl0(self.output["m0"], self.output["s0"]))))
        if self._ctx is None:
            self._ctx = Context(self.model._model_id, self._method, self.dim_d, self.dim_n, float(self.fwd_ode.dt),
                                e0=self._e0[1], device=self.device, flags=self.flags, batch=self.batch, **inputs)
            self._ctx_key = key
        self._ctx.set_prior_energy(self._e0[1])
        return self._ctx

    def initialization(self):
        """Cubic-spline initial guess of (A_t, b_t), src/var_bayes/variational.py:73-139 (host-side)."""
        tw = self.model.time_window
        knots = [tw[0], *tw[self.obs_t], tw[-1]]
        if self.model.single_dim:
            vals = np.hstack((self.obs_y[0], self.obs_y, self.obs_y[-1]))
            a0 = 0.5 * (self.model.sigma / 0.25) * np.ones(self.dim_n)
            b0 = CubicSpline(knots, vals)(tw)
        else:
            vals = np.vstack((self.obs_y[0], self.obs_y, self.obs_y[-1]))
            mt0 = CubicSpline(knots, vals)(tw)
            a0 = np.zeros((self.dim_n, self.dim_d, self.dim_d))
            b0 = np.zeros((self.dim_n, self.dim_d))
            slope = np.diff(mt0, axis=0) / self.dt
            half_k = 0.5 * np.diag(self.model.sigma.diagonal() / (0.25 * np.eye(self.dim_d)).diagonal())
            for k in range(self.dim_n - 1):
                a0[k] = half_k
                b0[k] = slope[k] + a0[k].diagonal() * mt0[k]
            a0[-1] = half_k
            b0[-1] = a0[-1].diagonal() * mt0[-1]
        return np.concatenate((a0.ravel(), b0.ravel()))

    def free_energy(self, x):
        """E0 + Esde + Eobs at x; leaves (m, S, lam, Psi, <f>) resident on the device."""
        f = self._context().free_energy(np.asarray(x, dtype=float))
        self._stale = {"mt", "st", "Efx", "Edf", "lamt", "psit"}
        return f

    def gradient(self, x, eval_fun=False):
        """Gradient of the Lagrangian w.r.t. (A_t, b_t), scaled by dt (variational.py:202-289)."""
        ctx = self._context()
        if eval_fun:
            _, g = ctx.sweep(np.asarray(x, dtype=float))
            self._stale = {"mt", "st", "Efx", "Edf", "lamt", "psit"}
            return g
        return ctx.gradient(None)

    def theta_gradient(self, x=None):
        """dF/dtheta at fixed (A_t, b_t), in the shape of model.theta (a float for OU / DW / L96, (3,) for L63; with batch > 1 a
        leading batch axis).  x=None: from the state of the last free_energy (like gradient(x, eval_fun=False)); else F is
        evaluated at x first."""
        if x is not None:
            self.free_energy(x)
        g = np.asarray(self._context().theta_gradient())
        if g.shape[-1] == 1:
            g = g[..., 0]
        return float(g) if g.ndim == 0 else g

    def posterior_kernel(self, anchors, kind="covariance", stride=1, x=None):
        """The covariance function of the posterior process between two grid times: a lagcov.LagCovariance (with batch > 1 a list, one per
        problem) holding K(k, s) = Cov[x_k, x_s] = Phi(k, s) S_s (kind "covariance") or the propagator Phi(k, s) (kind "propagator") for
        every anchor s in `anchors` and the grid indices k = 0, stride, 2 stride, ... >= s; its cov(k, s) / corr / joint / increment_var
        give the rest.  x=None: from the state of the last free_energy, which stays as it is; else F is evaluated at x first (the
        propagator reads A_t alone and only uploads x).  Deterministic: what thousands of sample_paths draws estimate."""
        xx = None if x is None else np.asarray(x, dtype=float)
        if xx is not None and kind == "covariance":
            self.free_energy(xx)
            xx = None
        res = self._context().lag_covariance(anchors, kind=kind, stride=stride, x=xx)
        if xx is not None:
            self._stale = {"mt", "st", "Efx", "Edf", "lamt", "psit"}
        return res.problem(0) if self.batch == 1 else [res.problem(p) for p in range(self.batch)]

    def sample_paths(self, n_paths, seed, stride=1, x=None, x0=None):
        """Draws from the posterior process dx = (-A_t x + b_t) dt + Sigma^1/2 dW by Euler-Maruyama on the grid: (n_paths, n_keep, D), or
        (n_paths, n_keep) for the 1-D models (with batch > 1 a leading batch axis), the grid points 0, stride, 2 stride, ...  x=None: the
        (A_t, b_t) of the last free_energy (like theta_gradient(); the cached state stays as it is).  x0=None: x_0 ~ N(m0, S0); else every
        path starts at x0.  The draws depend on (seed, problem, path, grid index, component) alone."""
        xx = None if x is None else np.asarray(x, dtype=float)
        out = self._context().sample_paths("posterior", n_paths, seed, stride=stride, x=xx, x0=x0)
        if self.model.single_dim:
            out = out[..., 0]
        return out[0] if self.batch == 1 else out

    def _path_weights(self, logw, start, paths, drawn):
        """One problem's record from its rows of Context.sample_paths_weighted: logw (n, 2), start (n, D), paths (n, n_keep, D) or None"""
        from .weights import PathWeights, init_term
        init = np.zeros(logw.shape[0])
        if drawn:
            init = init_term(start, self.kl0.mu0, self.kl0.tau0, self.output["m0"], self.output["s0"])
        if paths is not None and self.model.single_dim:
            paths = paths[..., 0]
        return PathWeights(init, logw[:, 0], logw[:, 1], paths)

    def importance_weights(self, n_paths, seed, x=None, x0=None, stride=None):
        """n_paths draws of the posterior process (sample_paths with the same arguments) weighted against the model SDE and the data: a
        weights.PathWeights (with batch > 1 a list, one per problem).  log w = init + path + obs; init = log N(x_0; mu0, tau0) -
        log N(x_0; m0, S0) with the prior of kl0, 0 when x0 is given.  stride=None: no path is stored -- the evidence-estimation mode, many
        paths and a tiny result; else the record carries the kept grid points.  x=None: the (A_t, b_t) of the last free_energy."""
        xx = None if x is None else np.asarray(x, dtype=float)
        paths, logw, start = self._context().sample_paths_weighted(n_paths, seed, stride=1 if stride is None else stride, x=xx, x0=x0,
                                                                   paths=stride is not None)
        out = [self._path_weights(logw[k], start[k], None if paths is None else paths[k], x0 is None) for k in range(logw.shape[0])]
        return out[0] if self.batch == 1 else out

    def _particle_record(self, res, k, n_obs=None):
        """One problem's ParticleFilterResult from row k of Context.particle_filter's dict, cut to its own n_obs observations"""
        from .particles import ParticleFilterResult
        m = res["ess"].shape[1] if n_obs is None else int(n_obs)
        cut = lambda a: None if a is None else a[k, :m]      # noqa: E731
        state, clouds = res["state"][k], cut(res["clouds"])
        if self.model.single_dim:
            state, clouds = state[..., 0], None if clouds is None else clouds[..., 0]
        return ParticleFilterResult(res["log_w"][k], state, cut(res["ess"]), cut(res["resampled"]), cut(res["ancestors"]), clouds)

    def _prior(self):
        d = self.dim_d
        return np.reshape(np.asarray(self.kl0.mu0, dtype=float), (1, d)), np.reshape(np.asarray(self.kl0.tau0, dtype=float), (1, d, d))

    def _particle_call(self, name, record, *args, x=None, late=None, **kwargs):
        """What the particle methods share: x as a float array, the prior of kl0, Context.<name>(*args, x=, prior=, **kwargs), and
        record(res, k, *late()) for every problem k of its dict -- one record with batch = 1, else their list.  late: what the records
        need beside the dict and can be made only behind the call, which has checked the arguments"""
        xx = None if x is None else np.asarray(x, dtype=float)
        res = getattr(self._context(), name)(*args, x=xx, prior=self._prior(), **kwargs)
        extra = late() if late else ()
        out = [record(res, k, *extra) for k in range(res["log_w"].shape[0])]
        return out[0] if self.batch == 1 else out

    def particle_filter(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, history=False):
        """A guided particle filter with the posterior process as its proposal: n_paths particles walk the recursion of sample_paths,
        take in their weight against the model SDE and the data observation by observation, and are resampled (systematic) whenever
        ESS < ess_fraction n_paths: a particles.ParticleFilterResult (with batch > 1 a list, one per problem).  The initial term uses the
        prior of kl0 (0 when x0 is given).  ess_fraction=0 never resamples: the weights of importance_weights().  history=True keeps the
        ancestors and the clouds at the observations (lineages()).  x=None: the (A_t, b_t) of the last free_energy.  From the first
        resampling on a particle depends on n_paths."""
        return self._particle_call("particle_filter", self._particle_record, n_paths, seed, ess_fraction=ess_fraction, x=x, x0=x0, history=history)

    def _statistics_record(self, res, k, n_obs=None):
        """One problem's PathStatistics from row k of Context.particle_statistics' dict, cut to its own n_obs observations"""
        from .particles import PathStatistics
        m = res["ess"].shape[1] if n_obs is None else int(n_obs)
        rows = None if res["stats"] is None else res["stats"][k]
        return PathStatistics(res["log_w"][k], res["mean"][k], float(self.fwd_ode.dt), self.dim_n - 1, self.model._model_id, res["ess"][k, :m],
                              res["resampled"][k, :m], rows)

    def particle_statistics(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, per_particle=False):
        """particle_filter with the same arguments, every particle carrying the path statistics (Q, G, H) of its lineage: a
        particles.PathStatistics (with batch > 1 a list, one per problem) with the weighted mean of the rows, reduced on the device, and
        -- per_particle=True -- the rows.  Its score(), theta_step() and expected_loglik() are the score of log p(y | theta, Sigma), the
        exact EM step in theta and the EM Q-function under the particles' smoothing distribution."""
        return self._particle_call("particle_statistics", self._statistics_record, n_paths, seed, ess_fraction=ess_fraction, x=x, x0=x0,
                                   per_particle=per_particle)

    def _events_record(self, res, k, levels, side, stride, n_obs=None):
        """One problem's PathEvents from row k of Context.particle_events' dict, cut to its own n_obs observations"""
        from .particles import PathEvents
        m = res["ess"].shape[1] if n_obs is None else int(n_obs)
        rows = None if res["rows"] is None else res["rows"][k]
        return PathEvents(res["log_w"][k], res["mean"][k], res["cdf"][k], levels, side, stride, self.dim_n, float(self.fwd_ode.dt), res["ess"][k, :m],
                          res["resampled"][k, :m], rows)

    def particle_events(self, n_paths, seed, levels, side=1, stride=1, ess_fraction=0.5, x=None, x0=None, per_particle=False):
        """particle_filter with the same arguments, every particle carrying the event records of its lineage: a particles.PathEvents (with
        batch > 1 a list, one per problem).  levels (D,) or a scalar, side +1 (above) or -1 (below) per component: the event of component j
        is side_j (x_j - levels_j) > 0.  prob_crossed, first_passage_cdf(), occupation_time and mean_extreme come from sums reduced on the
        device over all n_paths lineages (no path is stored or copied); per_particle=True also keeps the rows."""
        return self._particle_call("particle_events", lambda res, k, lev, sd: self._events_record(res, k, lev[k], sd[k], stride), n_paths, seed, levels,
                                   side=side, stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, per_particle=per_particle,
                                   late=lambda: (per_problem(levels, self.batch, self.dim_d), per_problem(side, self.batch, self.dim_d)))

    def _moments_record(self, res, k, stride, obs_t=None):
        """One problem's SmoothingMoments from row k of Context.particle_moments' dict, cut to its own observations obs_t"""
        from .particles import SmoothingMoments
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return SmoothingMoments(res["log_w"][k], res["moments"][k], stride, self.dim_n, t, res["lineage_ess"][k, :t.size + 1],
                                res["ess"][k, :t.size], res["resampled"][k, :t.size], self.model.single_dim)

    def particle_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """The smoothing mean and variance on the time grid from particle_filter with the same arguments: a particles.SmoothingMoments
        (with batch > 1 a list, one per problem) -- mean, second, var, std at the grid indices 0, stride, ... under the filter's
        genealogy, reduced on the device (no path is stored or copied), and lineage_ess, the number of distinct lineages each stretch
        between two observations rests on in effect.  What to hold m_t and S_t against."""
        return self._particle_call("particle_moments", lambda res, k: self._moments_record(res, k, stride), n_paths, seed, stride=stride,
                                   ess_fraction=ess_fraction, x=x, x0=x0)

    def _backward_moments_record(self, res, k, stride, obs_t=None):
        """One problem's BackwardSmoothingMoments from row k of Context.particle_backward_moments' dict, cut to its own observations obs_t"""
        from .particles import BackwardSmoothingMoments
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return BackwardSmoothingMoments(res["log_w"][k], res["moments"][k], stride, self.dim_n, t, res["smoothing_ess"][k, :t.size + 1],
                                        res["weights"][k, :t.size + 1], res["ess"][k, :t.size], res["resampled"][k, :t.size], self.model.single_dim)

    def backward_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """particle_moments with the weights of the marginal backward smoother: a particles.BackwardSmoothingMoments (with batch > 1 a list,
        one per problem) -- mean, second, var, std on the grid, smoothing_ess per stretch and the weights themselves.  At every observation
        where the cloud was resampled the weights of the stretch before it come from all n_paths particles of the stored cloud (filter
        weight times model transition density, normalised per successor), the expectation of backward_paths' draw: early stretches keep a
        variance where the genealogy's has collapsed to zero -- on clouds that overlap (the 1-D and 3-D models with many observations).
        Where the particles lie many transition widths apart the result is particle_moments'."""
        return self._particle_call("particle_backward_moments", lambda res, k: self._backward_moments_record(res, k, stride), n_paths, seed,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0)

    def _covariance_record(self, res, k, stride, obs_t=None):
        """One problem's SmoothingCovariance from row k of Context.particle_covariance's dict, cut to its own observations obs_t"""
        from .particles import SmoothingCovariance
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return SmoothingCovariance(res["log_w"][k], res["mean"][k], res["second"][k], stride, self.dim_n, t, res["lineage_ess"][k, :t.size + 1],
                                   res["ess"][k, :t.size], res["resampled"][k, :t.size], self.model.single_dim)

    def particle_covariance(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """The smoothing mean and full covariance matrices on the time grid from particle_filter with the same arguments: a
        particles.SmoothingCovariance (with batch > 1 a list, one per problem) -- mean, second, cov, var, corr at the grid indices 0, stride,
        ... under the filter's genealogy, reduced on the device, and lineage_ess as particle_moments has it.  What to hold the whole of
        S_t against, its off-diagonal entries included; gaussian(dim_n - 1) is the filtering Gaussian a following window starts from."""
        return self._particle_call("particle_covariance", lambda res, k: self._covariance_record(res, k, stride), n_paths, seed, stride=stride,
                                   ess_fraction=ess_fraction, x=x, x0=x0)

    def _kernel_record(self, res, k, anchors, stride, obs_t=None):
        """One problem's SmoothingLagCovariance from row k of Context.particle_lag_covariance's dict, cut to its own observations obs_t"""
        from .particles import SmoothingLagCovariance
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return SmoothingLagCovariance(res["log_w"][k], res["mean"][k], res["cross"][k], anchors, stride, self.dim_n, t,
                                      res["lineage_ess"][k, :t.size + 1], res["ess"][k, :t.size], res["resampled"][k, :t.size], self.model.single_dim)

    def particle_kernel(self, n_paths, seed, anchors, stride=1, ess_fraction=0.5, x=None, x0=None):
        """The particle estimate of the posterior's covariance function, Cov[x_k, x_s | y] for every kept grid index k and every anchor s,
        from particle_filter with the same arguments: a particles.SmoothingLagCovariance (with batch > 1 a list, one per problem) -- cov,
        corr, increment_var, autocorrelation and joint(), named and called as lagcov.LagCovariance's -- from the two-time moments of all
        n_paths lineages, contracted on the device; only the moments are copied.  anchors: strictly increasing grid indices, multiples
        of stride.  What to hold posterior_kernel()'s K(k, s) against; lineage_ess says how few lineages the early stretches rest on."""
        return self._particle_call("particle_lag_covariance", lambda res, k: self._kernel_record(res, k, anchors, stride), n_paths, seed, anchors,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0)

    def _marginals_record(self, res, k, levels, stride, obs_t=None):
        """One problem's SmoothingMarginals from row k of Context.particle_marginals' dict, cut to its own observations obs_t"""
        from .particles import SmoothingMarginals
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return SmoothingMarginals(res["log_w"][k], levels, res["mass"][k], res["q_final"][k], stride, self.dim_n, t, res["lineage_ess"][k, :t.size + 1],
                                  res["ess"][k, :t.size], res["resampled"][k, :t.size], self.model.single_dim)

    def _gaussian_ladders(self, x, n_levels, width):
        """(ladders (batch, D, n_levels), None): particles.posterior_ladders of the Gaussian posterior at x -- F is evaluated at x first, so
        that the call behind it reads the cached state -- or, x=None, of the last free_energy.  (ProblemBatch's free_energy stacks x.)"""
        from .particles import posterior_ladders
        if x is not None:
            self.free_energy(x)
        return posterior_ladders(self._context(), n_levels, width), None

    def particle_marginals(self, n_paths, seed, levels=None, stride=1, ess_fraction=0.5, x=None, x0=None, n_levels=31, width=4.0):
        """The smoothing marginals on the time grid from particle_filter with the same arguments: a particles.SmoothingMarginals (with
        batch > 1 a list, one per problem) -- per component a histogram of x_k | y over a ladder of levels at the grid indices 0, stride,
        ..., counted on the device in integer arithmetic (no path is stored or copied): cdf(), hist(), exceedance(), quantile(), band() and
        modes().  levels: (L,), (D, L) or (batch, D, L), strictly increasing, L <= 63; None: per component n_levels uniform levels over
        m_t -+ width sqrt(S_t) of the Gaussian posterior at x (particles.gaussian_ladder).  What m_t and S_t cannot say: whether the
        marginal is bimodal, and where its quantiles lie against m_t -+ 1.64 sqrt(S_t)."""
        if levels is None:
            levels, x = self._gaussian_ladders(x, n_levels, width)
        return self._particle_call("particle_marginals", lambda res, k, lev: self._marginals_record(res, k, lev[k], stride), n_paths, seed, levels,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0,
                                   late=lambda: (self._context()._ladder_input(levels)[0],))

    def _paths_record(self, res, k, stride, drawn, obs_t=None, method="genealogy"):
        """One problem's SmoothingPaths from row k of Context.particle_paths' (or particle_backward_paths') dict, cut to its own observations obs_t"""
        from .particles import SmoothingPaths
        t = np.asarray(self._inputs()["obs_t"] if obs_t is None else obs_t).ravel()
        return SmoothingPaths(res["log_w"][k], res["paths"][k], res["slots"][k, :t.size + 1], stride, self.dim_n, t, res["ess"][k, :t.size],
                              res["resampled"][k, :t.size], drawn, self.model.single_dim, method=method)

    def particle_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, slots=None):
        """n_draw whole smoothing trajectories on the time grid from particle_filter with the same arguments: a particles.SmoothingPaths
        (with batch > 1 a list, one per problem) -- paths (n_draw, n_keep, D) at the grid indices 0, stride, ..., equally weighted draws
        from the filter's genealogy (slots=None) or the lineages of the given final slots, and the slot of every trajectory in every
        stretch.  Only the n_draw trajectories are walked again and copied.  On collapsing clouds the early stretches of all
        trajectories coincide: distinct() says how many are left."""
        return self._particle_call("particle_paths", lambda res, k: self._paths_record(res, k, stride, slots is None), n_paths, seed, n_draw,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, slots=slots)

    def backward_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, slots=None):
        """n_draw whole smoothing trajectories by backward simulation (forward filtering, backward simulation) through the clouds of
        particle_filter with the same arguments: a particles.SmoothingPaths with method "backward" (with batch > 1 a list), laid out as
        particle_paths'.  At every observation where the cloud was resampled a trajectory draws the slot it came from among all n_paths
        particles, in proportion to filter weight times model transition density, instead of following its ancestor: the early stretches
        keep more distinct paths than the genealogy leaves.  Between two observations a trajectory is still its slot's own path, so
        distinct() is bounded by the distinct slots chosen."""
        return self._particle_call("particle_backward_paths", lambda res, k: self._paths_record(res, k, stride, slots is None, method="backward"),
                                   n_paths, seed, n_draw, stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, slots=slots)

    def _forecast_record(self, res, k, horizon, stride, drawn):
        """One problem's Forecast from row k of Context.particle_forecast's dict"""
        from .particles import Forecast
        return Forecast(res["log_w"][k], res["moments"][k], res["members"][k], res["slots"][k], res["state_end"][k], res["index0"], horizon, stride,
                        float(self.fwd_ode.dt), float(np.ravel(self.model.time_window)[0]), drawn, self.model.single_dim)

    def _forecast(self, context, prior, horizon, n_paths, seed, stride, n_draw, ess_fraction, xx, x0, source, cloud, log_w, index0, slots):
        """Context.particle_forecast's dict for forecast(), here and in a batch of members like this one (context, prior: how to get them):
        the source of the cloud chosen, a given cloud of a 1-D model given its component axis"""
        if source not in ("filter", "posterior"):
            raise ValueError(f" Unknown source of the forecast -> {source}")
        if source == "posterior":      # the end points of the posterior process's paths, equally weighted, at the last grid index
            if cloud is not None or n_paths is None:
                raise ValueError(" forecast: source='posterior' draws its own cloud of n_paths particles.")
            ends = context().sample_paths("posterior", n_paths, seed, stride=self.dim_n - 1 if self.dim_n > 1 else 1, x=xx, x0=x0)
            cloud, log_w, index0 = ends[:, :, -1, :], None, self.dim_n - 1
        if cloud is None:
            return context().particle_forecast(horizon, n_paths, seed, stride=stride, n_draw=n_draw, ess_fraction=ess_fraction, x=xx, x0=x0,
                                               slots=slots, prior=prior())
        cloud = np.asarray(cloud, dtype=float)
        cloud = cloud.reshape(cloud.shape + (1,)) if self.model.single_dim and cloud.shape[-1:] != (1,) else cloud
        return context().particle_forecast(horizon, seed=seed, stride=stride, n_draw=n_draw, cloud=cloud, log_w=log_w, index0=index0, slots=slots)

    def forecast(self, horizon, n_paths=None, seed=0, stride=1, n_draw=0, ess_fraction=0.5, x=None, x0=None, source="filter", cloud=None,
                 log_w=None, index0=None, slots=None):
        """The forecast past the window: a weighted cloud carried `horizon` steps forward under the model SDE on the device, a
        particles.Forecast (with batch > 1 a list, one per problem) with mean and var on the forecast grid, n_draw member trajectories
        (slots=None: of slots drawn from the weights) and the cloud at the end.  source="filter": the final cloud of particle_filter with
        the same n_paths, seed, ess_fraction, x, x0, taken where it lies on the device; source="posterior": the end points of
        sample_paths(n_paths, seed, x=x, x0=x0), equally weighted.  cloud (n, D), log_w (n,), index0: a given cloud at that absolute grid
        index (None: the last one of the window) -- the state and log_w of an earlier forecast continue it."""
        xx = None if x is None else np.asarray(x, dtype=float)
        res = self._forecast(self._context, self._prior, horizon, n_paths, seed, stride, n_draw, ess_fraction, xx, x0, source, cloud, log_w, index0,
                             slots)
        out = [self._forecast_record(res, k, horizon, stride, slots is None) for k in range(res["moments"].shape[0])]
        return out[0] if self.batch == 1 else out

    def particle_fit_theta(self, n_paths, seed, iters, ess_fraction=0.5, refit=True, pooled=False):
        """Particle EM for the drift parameters (ProblemBatch.particle_fit_theta on a batch of one): (theta, trace), theta in the shape of
        model.theta."""
        from .batch import ProblemBatch
        pb = ProblemBatch([self], device=self.device, flags=self.flags)
        try:
            theta, trace = pb.particle_fit_theta(n_paths, seed, iters, ess_fraction=ess_fraction, refit=refit, pooled=pooled)
        finally:
            pb.close()
        theta = theta[0]
        return (float(theta[0]) if theta.size == 1 else theta), trace

    def particle_gibbs(self, n_paths, seed, iters, burn=0, thin=1, ess_fraction=0.5, sample_theta=True, theta_prior=None, x=None):
        """Particle Gibbs with ancestor sampling for the joint posterior of theta and the path (ProblemBatch.particle_gibbs on a batch of
        one): a particles.GibbsChain.  x: the fixed proposal (A_t, b_t), initialization() by default."""
        from .batch import ProblemBatch
        pb = ProblemBatch([self], device=self.device, flags=self.flags)
        try:
            chain = pb.particle_gibbs(n_paths, seed, iters, burn=burn, thin=thin, ess_fraction=ess_fraction, sample_theta=sample_theta,
                                      theta_prior=theta_prior, x=None if x is None else np.asarray(x, dtype=float).reshape(1, -1))[0]
        finally:
            pb.close()
        return chain

    def fit_theta(self, x0, rounds, options=None):
        """Variational EM for the drift parameters (ProblemBatch.fit_theta on a batch of one): (x, F, theta, trace), theta in the
        shape of model.theta, trace["F"] of shape (rounds, 2, 1)."""
        from .batch import ProblemBatch
        pb = ProblemBatch([self], device=self.device, flags=self.flags)
        try:
            x, f, theta, trace = pb.fit_theta(np.asarray(x0, dtype=float).reshape(1, -1), rounds, options)
        finally:
            pb.close()
        theta = theta[0]
        return x[0], float(f[0]), (float(theta[0]) if theta.size == 1 else theta), trace

    def sweep(self, x):
        """(F, grad) in one call: what SCG's df(x, eval_fun=True) evaluates."""
        f, g = self._context().sweep(np.asarray(x, dtype=float))
        self._stale = {"mt", "st", "Efx", "Edf", "lamt", "psit"}
        return f, g

    def device_scg(self, *options):
        """SCG with x, d and the gradients resident in HBM (scg.DeviceSCG); `batch` problems advance in lock step."""
        from .scg import DeviceSCG
        self._stale = {"mt", "st", "Efx", "Edf", "lamt", "psit"}
        return DeviceSCG(self._context(), *options)

    @property
    def arg_out(self):
        """The reference's output dictionary (m0, s0, mt, st, Efx, Edf, lamt, psit), fetched lazily."""
        for key in sorted(self._stale):
            val = self._ctx.fetch(key)
            if self.model.single_dim:
                val = val.reshape(self.dim_n)
            self.output[key] = val
        self._stale = set()
        return self.output
