"""
ProblemBatch: many independent smoothing problems of one model in ONE batched device context.

Each member is a `VarGP` wired on its own dataset (its own sample path, observations and initial moments, as
`Simulation.setup` builds them).  The members must share everything a context shares -- the model class, theta, Sigma,
dt, Np, the integration method, R, H and the observation count M -- and may differ in what `Context.set_problem_data`
takes per problem: the observation times and values, m0, S0 and E0 = KL(q0||p0) (each computed with the member's own
`kl0`).  The batch then runs at the throughput of the batched kernels instead of one context per dataset.
With own_parameters=True theta and Sigma leave the shared list: each member's own model.theta / model.sigma goes to
`Context.set_problem_params` (a parameter study: one dataset at many (theta, Sigma) points).
With own_observations=True the observation count M, R and H leave it too: the context holds rows of max_p M_p observations,
shorter datasets are padded, and each member's own count, R and H go to `Context.set_problem_obs_model` (recordings of
different length, instruments of different noise, sensors that see different components).

    pb = ProblemBatch([vgp_a, vgp_b, ...])
    x, f, stats = pb.optimise(pb.initialization(), {"max_it": 500})
    out = pb.result(1)            # problem 1's result dictionary, as save_results writes it
"""
import numpy as np

from ._lib import Context, per_problem

__all__ = ["ProblemBatch", "theta_mstep", "stack_observations"]


def theta_mstep(theta, g0, g1, pooled=False):
    """
    The exact M-step in theta at fixed (A_t, b_t).  F is quadratic in theta there with a diagonal Hessian, so with g0 = dF/dtheta at
    theta and g1 = dF/dtheta at theta + 1 (every component raised by one) the curvature is h = g1 - g0 and the minimiser
    theta - g0 / h, component-wise.  theta, g0, g1: (B, n_theta).  pooled=True: the B problems share one theta (many datasets of
    one system), the objective is the sum of their F, and every row moves by sum_p g0 / sum_p h.  Returns (B, n_theta).
    """
    theta, g0, g1 = (np.atleast_2d(np.asarray(v, dtype=float)) for v in (theta, g0, g1))
    h = g1 - g0
    if pooled:
        step = np.broadcast_to(g0.sum(axis=0) / h.sum(axis=0), theta.shape)
    else:
        step = g0 / h
    return theta - step


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def stack_observations(rows):
    """
    The observation inputs of B members with their own counts, as one context takes them.  rows: B dictionaries with obs_t (M_p,),
    obs_y (M_p, D) or (M_p,), obs_noise (D, D) and obs_h (D, D) or None.  Returns a dictionary: n_obs (B,) int32, obs_t (B, M) int64 and
    obs_y (B, M, D) with M = max_p M_p -- the entries beyond a member's count hold -1 and NaN, which no kernel may read --, obs_noise
    (B, D, D), obs_h (B, D, D) or None when no member has an operator (a member without one among others gets the identity).
    """
    n_obs = np.array([np.asarray(r["obs_t"]).size for r in rows], dtype=np.int32)
    if n_obs.min() < 1:
        raise ValueError(" ProblemBatch: every problem needs at least one observation.")
    B, M = len(rows), int(n_obs.max())
    D = np.asarray(rows[0]["obs_noise"]).shape[-1] if np.asarray(rows[0]["obs_noise"]).ndim else 1
    obs_t = np.full((B, M), -1, dtype=np.int64)
    obs_y = np.full((B, M, D), np.nan)
    for p, r in enumerate(rows):
        obs_t[p, :n_obs[p]] = np.asarray(r["obs_t"], dtype=np.int64).ravel()
        obs_y[p, :n_obs[p]] = np.asarray(r["obs_y"], dtype=float).reshape(n_obs[p], D)
    obs_noise = np.stack([np.asarray(r["obs_noise"], dtype=float).reshape(D, D) for r in rows])
    obs_h = None
    if any(r["obs_h"] is not None for r in rows):
        obs_h = np.stack([np.eye(D) if r["obs_h"] is None else np.asarray(r["obs_h"], dtype=float).reshape(D, D) for r in rows])
    return dict(n_obs=n_obs, obs_t=obs_t, obs_y=obs_y, obs_noise=obs_noise, obs_h=obs_h)


class ProblemBatch(object):

    def __init__(self, vgps, device=0, flags=0, own_parameters=False, own_observations=False) -> None:
        self.vgps = list(vgps)
        if not self.vgps:
            raise ValueError(" ProblemBatch: no problems given.")
        self.device, self.flags = device, int(flags)
        self.own_parameters = bool(own_parameters)
        self.own_observations = bool(own_observations)
        self.B = len(self.vgps)
        self._check_shared()
        first = self.vgps[0]
        self.dim_n, self.dim_d = first.dim_n, first.dim_d
        self.len_x = self.dim_n * self.dim_d * (self.dim_d + 1)
        self._ctx, self._ctx_key = None, None
        self._x = self._f = None
        self._outputs = None        # (context key, x, F, {key: (B, ...) array}) of the last result() evaluation

    # ------------------------------------------------------------------------------------------
    def _shared(self, vgp):
        """What one context holds for all of its problems, in the order the fields are compared."""
        inp = vgp._inputs()
        fields = [("model", type(vgp.model)), ("theta", inp["theta"]), ("sigma", inp["sigma"]), ("dt", float(vgp.fwd_ode.dt)),
                  ("Np", vgp.dim_n), ("method", vgp._method), ("R", inp["obs_noise"]), ("H", inp["obs_h"]),
                  ("M", int(inp["obs_t"].size))]
        if self.own_parameters:     # (theta and sigma go to Context.set_problem_params instead)
            fields = [f for f in fields if f[0] not in ("theta", "sigma")]
        if self.own_observations:   # (R, H and the count go to Context.set_problem_obs_model instead)
            fields = [f for f in fields if f[0] not in ("R", "H", "M")]
        return fields

    def _check_shared(self):
        ref = self._shared(self.vgps[0])
        label = {"model": "the model class", "M": "the observation count M"}
        names = [label.get(name, name) for name, _ in ref]
        shared = ", ".join(names[:-1]) + " and " + names[-1]
        for k, vgp in enumerate(self.vgps[1:], start=1):
            for (name, a), (_, b) in zip(ref, self._shared(vgp)):
                equal = (a is b) if name == "model" else (a == b if isinstance(a, (int, float, str)) else _same(a, b))
                if not equal:
                    raise ValueError(f" ProblemBatch: problem {k} differs from problem 0 in '{name}'; a batch shares {shared}.")

    def _per_problem(self):
        """The per-problem inputs of every member, read from the objects NOW, and the priors E0 depends on."""
        rows = [vgp._inputs() for vgp in self.vgps]
        prior = tuple(np.asarray(getattr(v.kl0, k, 0.0), dtype=float).tobytes() for v in self.vgps for k in ("mu0", "tau0"))
        if self.own_observations:   # padded rows of max_p M_p observations, every member's own count, R and H
            pp = {k: v for k, v in stack_observations(rows).items() if v is not None}
        else:
            obs_t = np.stack([r["obs_t"] for r in rows])
            pp = dict(obs_t=obs_t, obs_y=np.stack([r["obs_y"].reshape(obs_t.shape[1], -1) for r in rows]))
        pp.update(m0=np.stack([r["m0"] for r in rows]), s0=np.stack([r["s0"] for r in rows]))
        if self.own_parameters:     # every member's own model.theta / model.sigma (and with them the context key)
            pp["theta"] = np.stack([r["theta"] for r in rows])
            pp["sigma"] = np.stack([r["sigma"] for r in rows])
        return pp, prior

    def _context(self):
        # like VarGP._context: a context built from inputs that have changed since is rebuilt (the shared ones are checked again)
        self._check_shared()
        pp, prior = self._per_problem()
        # (own observations: the member with the most observations lends the shared row, which vgpa_create validates whole)
        shared = self.vgps[int(np.argmax(pp["n_obs"])) if self.own_observations else 0]._inputs()
        key = (shared["theta"].tobytes(), shared["sigma"].tobytes(), shared["obs_noise"].tobytes(),
               None if shared["obs_h"] is None else shared["obs_h"].tobytes(), prior) + tuple(pp[k].tobytes() for k in sorted(pp))
        if self._ctx is not None and key == self._ctx_key:
            return self._ctx
        self.close()
        pp["e0"] = np.array([float(np.asarray(v.kl0(v.output["m0"], v.output["s0"]))) for v in self.vgps])
        # the shared fields of the context come from problem 0; every per-problem field is replaced below.  Observation
        # times stay shared when every member observes at the same grid points (the only form above D = 64).
        ctx = Context(self.vgps[0].model._model_id, self.vgps[0]._method, self.dim_d, self.dim_n, float(self.vgps[0].fwd_ode.dt),
                      e0=float(pp["e0"][0]), batch=self.B, device=self.device, flags=self.flags, **shared)
        if self.own_observations:   # (the counts first: the padded rows below are then validated up to each member's own count)
            ctx.set_problem_obs_model(n_obs=pp["n_obs"], obs_noise=pp["obs_noise"], obs_h=pp.get("obs_h"))
        same_t = bool(np.all(pp["obs_t"] == pp["obs_t"][:1]))
        ctx.set_problem_data(obs_t=None if same_t else pp["obs_t"], obs_y=pp["obs_y"], m0=pp["m0"], s0=pp["s0"], e0=pp["e0"])
        if self.own_parameters:
            ctx.set_problem_params(theta=pp["theta"], sigma=pp["sigma"])
        self._ctx, self._ctx_key = ctx, key
        return ctx

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
        self._ctx, self._ctx_key = None, None

    # ------------------------------------------------------------------------------------------
    def _stack(self, x):
        x = np.asarray(x, dtype=float)
        if x.size != self.B * self.len_x:
            raise ValueError(f" ProblemBatch: x has {x.size} entries, expected {self.B} x {self.len_x}")
        return x.reshape(self.B, self.len_x)

    def initialization(self):
        """(B, len_x): every member's own cubic-spline initial guess (VarGP.initialization)."""
        return np.stack([vgp.initialization() for vgp in self.vgps])

    def free_energy(self, x):
        """(B,) free energies; leaves the state of every problem resident for gradient() / result()."""
        f = self._context().free_energy(self._stack(x))
        return np.atleast_1d(np.asarray(f, dtype=float))

    def gradient(self, x=None):
        """(B, len_x); x=None: from the state of the last free_energy (VarGP.gradient(x, eval_fun=False))."""
        g = self._context().gradient(None if x is None else self._stack(x))
        return np.asarray(g).reshape(self.B, self.len_x)

    def sweep(self, x):
        """(F (B,), gradient (B, len_x)) in one call."""
        f, g = self._context().sweep(self._stack(x))
        return np.atleast_1d(np.asarray(f, dtype=float)), np.asarray(g).reshape(self.B, self.len_x)

    def theta_gradient(self, x=None):
        """(B, n_theta) dF/dtheta at fixed (A_t, b_t); x=None: from the state of the last free_energy, else F is evaluated at x
        first.  Every member's own theta / Sigma / data are honoured."""
        if x is not None:
            self.free_energy(x)
        return np.asarray(self._context().theta_gradient(), dtype=float).reshape(self.B, -1)

    def posterior_kernel(self, anchors, kind="covariance", stride=1, x=None):
        """One lagcov.LagCovariance per member (VarGP.posterior_kernel): K(k, s) = Phi(k, s) S_s of the member's own posterior process, or
        its propagator Phi(k, s), from the anchors (shared by the batch) to the end of the grid.  x=None: the state of the last
        free_energy, which stays as it is; else F is evaluated at x first (the propagator only uploads x)."""
        xx = None if x is None else self._stack(x)
        if xx is not None and kind == "covariance":
            self.free_energy(xx)
            xx = None
        res = self._context().lag_covariance(anchors, kind=kind, stride=stride, x=xx)
        return [res.problem(p) for p in range(self.B)]

    def sample_paths(self, n_paths, seed, stride=1, x=None, x0=None, kind="posterior"):
        """(B, n_paths, n_keep, D) Euler-Maruyama paths of every member's posterior process (kind="model": of its model SDE, which takes no
        x), each with its own data, prior, theta and Sigma.  x=None: the x of the last free_energy, whose cached state stays as it is.
        x0 (B, D): given starts; None: x_0 ~ N(m0_p, S0_p).  Problem p's draws do not depend on the rest of the batch."""
        xx = None if x is None else self._stack(x)
        return self._context().sample_paths(kind, n_paths, seed, stride=stride, x=xx, x0=x0)

    def importance_weights(self, n_paths, seed, x=None, x0=None, stride=None):
        """One weights.PathWeights per member: n_paths draws of its posterior process weighted against its own model SDE and data
        (VarGP.importance_weights), the init term from the member's own prior (mu0, tau0) and (m0, S0); 0 when x0 (B, D) is given.
        stride=None: no path is stored."""
        xx = None if x is None else self._stack(x)
        paths, logw, start = self._context().sample_paths_weighted(n_paths, seed, stride=1 if stride is None else stride, x=xx, x0=x0,
                                                                   paths=stride is not None)
        return [v._path_weights(logw[k], start[k], None if paths is None else paths[k], x0 is None) for k, v in enumerate(self.vgps)]

    def _prior(self):
        """(mu0 (B, D), tau0 (B, D, D)): every member's own prior, stacked"""
        mu, tau = zip(*(v._prior() for v in self.vgps))
        return np.stack([m[0] for m in mu]), np.stack([t[0] for t in tau]).reshape(self.B, self.vgps[0].dim_d, self.vgps[0].dim_d)

    def _particle_call(self, name, record, *args, x=None, late=None, **kwargs):
        """What the particle methods share: x stacked, the members' priors, Context.<name>(*args, x=, prior=, **kwargs), and
        record(member, res, k, *late()) for every member k.  late: what the records need beside the dict and can be made only behind the
        call, which has checked the arguments"""
        xx = None if x is None else self._stack(x)
        prior = self._prior()
        res = getattr(self._context(), name)(*args, x=xx, prior=prior, **kwargs)
        extra = late() if late else ()
        return [record(v, res, k, *extra) for k, v in enumerate(self.vgps)]

    def particle_filter(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, history=False):
        """One particles.ParticleFilterResult per member (VarGP.particle_filter): each with its own data, observation times and count,
        prior, theta and Sigma; the histories are cut to the member's own observation count.  A member's result does not depend on the
        rest of the batch."""
        return self._particle_call("particle_filter", lambda v, res, k: v._particle_record(res, k, np.asarray(v._inputs()["obs_t"]).size),
                                   n_paths, seed, ess_fraction=ess_fraction, x=x, x0=x0, history=history)

    def particle_statistics(self, n_paths, seed, ess_fraction=0.5, x=None, x0=None, per_particle=False):
        """One particles.PathStatistics per member (VarGP.particle_statistics): the filter of particle_filter with the same arguments, each
        particle carrying the path statistics of its lineage under the member's own theta, Sigma, data and observation model."""
        return self._particle_call("particle_statistics", lambda v, res, k: v._statistics_record(res, k, np.asarray(v._inputs()["obs_t"]).size),
                                   n_paths, seed, ess_fraction=ess_fraction, x=x, x0=x0, per_particle=per_particle)

    def particle_events(self, n_paths, seed, levels, side=1, stride=1, ess_fraction=0.5, x=None, x0=None, per_particle=False):
        """One particles.PathEvents per member (VarGP.particle_events): the filter of particle_filter with the same arguments, each particle
        carrying the event records of its lineage.  levels and side: (B, D) for per-member levels and sides, or (D,) or a scalar for all."""
        return self._particle_call("particle_events",
                                   lambda v, res, k, lev, sd: v._events_record(res, k, lev[k], sd[k], stride, np.asarray(v._inputs()["obs_t"]).size),
                                   n_paths, seed, levels, side=side, stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, per_particle=per_particle,
                                   late=lambda: (per_problem(levels, self.B, self.dim_d), per_problem(side, self.B, self.dim_d)))

    def particle_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """One particles.SmoothingMoments per member (VarGP.particle_moments): the smoothing mean and second moment on the grid under the
        genealogy of the member's own filter, with its own data, observation times and count, prior, theta and Sigma."""
        return self._particle_call("particle_moments", lambda v, res, k: v._moments_record(res, k, stride), n_paths, seed, stride=stride,
                                   ess_fraction=ess_fraction, x=x, x0=x0)

    def backward_moments(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """One particles.BackwardSmoothingMoments per member (VarGP.backward_moments): particle_moments under the weights of the marginal
        backward smoother, each member with its own data, observation times and count, prior, theta and Sigma; a member's result does not
        depend on the rest of the batch."""
        return self._particle_call("particle_backward_moments", lambda v, res, k: v._backward_moments_record(res, k, stride), n_paths, seed,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0)

    def particle_covariance(self, n_paths, seed, stride=1, ess_fraction=0.5, x=None, x0=None):
        """One particles.SmoothingCovariance per member (VarGP.particle_covariance): the smoothing mean and full second-moment matrices on
        the grid under the genealogy of the member's own filter, with its own data, observation times and count, prior, theta and Sigma."""
        return self._particle_call("particle_covariance", lambda v, res, k: v._covariance_record(res, k, stride), n_paths, seed, stride=stride,
                                   ess_fraction=ess_fraction, x=x, x0=x0)

    def particle_kernel(self, n_paths, seed, anchors, stride=1, ess_fraction=0.5, x=None, x0=None):
        """One particles.SmoothingLagCovariance per member (VarGP.particle_kernel): Cov[x_k, x_s | y] between every kept grid index and the
        anchors -- shared by the members -- under the genealogy of the member's own filter."""
        return self._particle_call("particle_lag_covariance", lambda v, res, k: v._kernel_record(res, k, anchors, stride), n_paths, seed, anchors,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0)

    def particle_marginals(self, n_paths, seed, levels=None, stride=1, ess_fraction=0.5, x=None, x0=None, n_levels=31, width=4.0):
        """One particles.SmoothingMarginals per member (VarGP.particle_marginals): per component a histogram of x_k | y over a ladder of
        levels on the grid under the genealogy of the member's own filter.  levels: (B, D, L) for per-member ladders, or (D, L) or (L,) for
        all; None: every member's own particles.gaussian_ladder of its Gaussian posterior at x."""
        if levels is None:
            from .particles import posterior_ladders
            if x is not None:      # (F at x first: the call behind it reads the cached state)
                self.free_energy(x)
            levels, x = posterior_ladders(self._context(), n_levels, width), None
        return self._particle_call("particle_marginals", lambda v, res, k, lev: v._marginals_record(res, k, lev[k], stride), n_paths, seed, levels,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0,
                                   late=lambda: (self._context()._ladder_input(levels)[0],))

    def particle_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, slots=None):
        """One particles.SmoothingPaths per member (VarGP.particle_paths): n_draw whole smoothing trajectories from the genealogy of the
        member's own filter, with its own data, observation times and count, prior, theta and Sigma."""
        return self._particle_call("particle_paths", lambda v, res, k: v._paths_record(res, k, stride, slots is None), n_paths, seed, n_draw,
                                   stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, slots=slots)

    def backward_paths(self, n_paths, seed, n_draw, stride=1, ess_fraction=0.5, x=None, x0=None, slots=None):
        """One particles.SmoothingPaths per member (VarGP.backward_paths): n_draw whole smoothing trajectories drawn backwards through the
        clouds of the member's own filter, with its own data, observation times and count, prior, theta and Sigma."""
        return self._particle_call("particle_backward_paths", lambda v, res, k: v._paths_record(res, k, stride, slots is None, method="backward"),
                                   n_paths, seed, n_draw, stride=stride, ess_fraction=ess_fraction, x=x, x0=x0, slots=slots)

    def forecast(self, horizon, n_paths=None, seed=0, stride=1, n_draw=0, ess_fraction=0.5, x=None, x0=None, source="filter", cloud=None,
                 log_w=None, index0=None, slots=None):
        """One particles.Forecast per member (VarGP.forecast): every member's cloud -- its own filter's final one, the end points of its
        posterior process's paths (source="posterior") or the given cloud (B, n, D) with log_w (B, n) at index0 -- carried `horizon` steps
        forward under its own theta and Sigma."""
        xx = None if x is None else self._stack(x)
        res = self.vgps[0]._forecast(self._context, self._prior, horizon, n_paths, seed, stride, n_draw, ess_fraction, xx, x0, source, cloud, log_w,
                                     index0, slots)
        return [v._forecast_record(res, k, horizon, stride, slots is None) for k, v in enumerate(self.vgps)]

    def particle_fit_theta(self, n_paths, seed, iters, ess_fraction=0.5, refit=True, pooled=False, x0=None, options=None):
        """
        Particle EM for the drift parameters under the smoothing distribution of the Euler-discretised model, free of the variational
        bias of fit_theta.  Per iteration i: (1) refit=True: optimise (A_t, b_t) from the current x at the current theta -- the posterior
        process is the proposal, the better it fits the fewer particles are needed; (2) particle_statistics(n_paths, seed + i); (3)
        theta <- theta + score / information (PathStatistics.theta_step), each member with its own Sigma.  pooled=True: the members share
        one theta and move by sum_p score / sum_p information, as theta_mstep(pooled=True).  x0 (B, len_x): the first (A_t, b_t),
        initialization() by default.  The new theta is written to every member's model.theta.
        There is no Sigma step: paths imputed at a fixed Sigma have quadratic variation Sigma T as dt -> 0, so Sigma <- E[Q] / n_steps
        barely moves (particles.py).
        Returns (theta (B, n_theta), trace) with trace["theta"] (iters + 1, B, n_theta): theta before the first and after every step,
        trace["log_evidence"] (iters, B): the evidence estimate at the theta each step started from, trace["score"] and
        trace["information"] (iters, B, n_theta), trace["x"] (iters, B, len_x): the (A_t, b_t) each step's particles were proposed from.
        """
        if self.B > 1 and not pooled and not self.own_parameters:
            raise ValueError(" ProblemBatch.particle_fit_theta: a batch that shares one theta moves it by the pooled step (pooled=True), "
                             "or every member keeps its own (own_parameters=True).")
        x = self.initialization() if x0 is None else self._stack(x0).copy()
        trace = {"theta": [self._theta_rows()], "x": [], "log_evidence": [], "score": [], "information": []}
        for it in range(int(iters)):
            if refit:
                x, _, _ = self.optimise(x, options)
                x = np.array(x, dtype=float)
            recs = self.particle_statistics(n_paths, int(seed) + it, ess_fraction=ess_fraction, x=x)
            sig = [np.asarray(v._inputs()["sigma"], dtype=float).reshape(self.dim_d, self.dim_d).diagonal() for v in self.vgps]
            trace["x"].append(x.copy())
            score = np.stack([r.score(s) for r, s in zip(recs, sig)])
            info = np.stack([r.information(s) for r, s in zip(recs, sig)])
            step = np.broadcast_to(score.sum(axis=0) / info.sum(axis=0), score.shape) if pooled else score / info
            new = self._theta_rows() + step
            for vgp, row in zip(self.vgps, new):
                vgp.model.theta = float(row[0]) if row.size == 1 else row.copy()
            trace["theta"].append(new)
            trace["log_evidence"].append([r.log_evidence() for r in recs])
            trace["score"].append(score)
            trace["information"].append(info)
        for key in trace:
            trace[key] = np.asarray(trace[key])
        return self._theta_rows(), trace

    def particle_gibbs(self, n_paths, seed, iters, burn=0, thin=1, ess_fraction=0.5, sample_theta=True, theta_prior=None, x=None):
        """
        Particle Gibbs with ancestor sampling: the posterior of theta jointly with the path, one particles.GibbsChain per member -- B
        chains in one context, each member's chain independent of the rest (its draws depend on the seed and its own index alone).
        Iteration 0 takes its reference from particle_paths(n_paths, seed, n_draw=1).  Iteration i: (1) Context.particle_conditional at the
        current theta from the current trajectory, with seed + 1 + i; (2) sample_theta=True: theta' ~ N(theta + s / I, 1 / I) given the new
        trajectory (particles.theta_conditional; theta_prior: None, flat, or (mean, precision) per component), its normals from
        numpy.random.Generator(PCG64([seed, i, member])) (particles.theta_draw), written to the member's model.theta as
        particle_fit_theta writes it (the models' own checks apply and nothing is clipped: where a short window says little, a prior keeps
        the draws admissible).  The trajectories of the iterations burn, burn + thin, ... are kept.
        (A_t, b_t) stay fixed at x (B, len_x) -- by default the point the last optimise() returned, else initialization() --: they are
        the proposal, not the model.  The chain is exact for the Euler-discretised model whatever the proposal and for any n_paths >= 2;
        a better proposal and more particles make it mix faster.
        """
        from .particles import GibbsChain, theta_conditional, theta_draw
        if self.B > 1 and sample_theta and not self.own_parameters:
            raise ValueError(" ProblemBatch.particle_gibbs: the members of a batch that shares one theta cannot each draw their own "
                             "(own_parameters=True, or sample_theta=False).")
        iters, burn, thin, seed = int(iters), int(burn), int(thin), int(seed)
        if iters < 1 or burn < 0 or thin < 1:
            raise ValueError(" ProblemBatch.particle_gibbs: iters and thin must be at least 1, burn at least 0.")
        xx = (self.initialization() if self._x is None else self._x.copy()) if x is None else self._stack(x).copy()
        d, v0, prior = self.dim_d, self.vgps[0], self._prior()
        dt, model = float(v0.fwd_ode.dt), v0.model._model_id
        first = self._context().particle_paths(n_paths, seed, 1, ess_fraction=ess_fraction, x=xx, prior=prior)["paths"][:, 0]
        ref = np.ascontiguousarray(first)
        theta, moved, kept, paths = [self._theta_rows()], [], [], []
        for it in range(iters):
            res = self._context().particle_conditional(ref, n_paths, seed + 1 + it, ess_fraction=ess_fraction, x=xx, prior=prior)
            new = res["trajectory"]
            moved.append(np.mean(np.any(new != ref, axis=2), axis=1))
            ref = new
            if it >= burn and (it - burn) % thin == 0:
                kept.append(it)
                paths.append(new.copy())
            rows = self._theta_rows()
            if sample_theta:
                for k, vgp in enumerate(self.vgps):
                    sig = np.asarray(vgp._inputs()["sigma"], dtype=float).reshape(d, d).diagonal()
                    mean, prec = theta_conditional(model, rows[k], new[k], dt, sig, theta_prior)
                    row = theta_draw(mean, prec, seed, it, k)
                    vgp.model.theta = float(row[0]) if row.size == 1 else row.copy()
            theta.append(self._theta_rows())
        theta, moved = np.asarray(theta), np.asarray(moved)
        stack = np.asarray(paths).reshape(len(kept), self.B, self.dim_n, d)
        return [GibbsChain(theta[:, k], stack[:, k], kept, moved[:, k], first[k], v.model.single_dim) for k, v in enumerate(self.vgps)]

    def _theta_rows(self):
        return np.stack([np.atleast_1d(np.asarray(v.model.theta, dtype=float)) for v in self.vgps])

    def fit_theta(self, x0, rounds, options=None):
        """
        Variational EM for the drift parameters.  Per round: (1) optimise (A_t, b_t) from the current x at the current theta;
        (2) g0 = dF/dtheta at the returned x; (3) g1 = the same at theta + 1 (a probe on the live context); (4) theta_mstep.
        own_parameters=True: every problem moves its own theta; otherwise the batch shares one theta and the step is pooled.
        The new theta is written to every member's model.theta (the models' own checks apply; nothing is clipped).
        Returns (x (B, len_x), F (B,), theta (B, n_theta), trace) with trace["F"] (rounds, 2, B): F after the E-step and after the
        M-step, trace["theta"] (rounds, B, n_theta): theta after each M-step, trace["g0"] / trace["g1"] (rounds, B, n_theta): the two
        gradients each M-step was computed from.
        """
        x = self._stack(x0).copy()
        trace = {"F": np.zeros((int(rounds), 2, self.B)), "theta": [], "g0": [], "g1": []}
        f = None
        for r in range(int(rounds)):
            x, _, _ = self.optimise(x, options)
            x = np.array(x, dtype=float)
            # (the state SCG leaves resident may belong to a rejected trial point: F and g0 at the returned x)
            trace["F"][r, 0] = self.free_energy(x)
            g0 = self.theta_gradient()
            theta = self._theta_rows()
            ctx = self._context()
            sigma = self._per_problem()[0]["sigma"] if self.own_parameters else None
            try:
                ctx.set_problem_params(theta=theta + 1.0, sigma=sigma)
                ctx.free_energy(x)
                g1 = np.asarray(ctx.theta_gradient(), dtype=float).reshape(self.B, -1)
            finally:
                self.close()            # (the probe's parameters are in force on that context: the next call builds a fresh one)
            new = theta_mstep(theta, g0, g1, pooled=not self.own_parameters)
            for vgp, row in zip(self.vgps, new):
                vgp.model.theta = float(row[0]) if row.size == 1 else row.copy()
            trace["theta"].append(new)
            trace["g0"].append(g0)
            trace["g1"].append(g1)
            f = self.free_energy(x)
            trace["F"][r, 1] = f
        for key in ("theta", "g0", "g1"):
            trace[key] = np.asarray(trace[key])
        self._x, self._f = x, f
        return x, f, self._theta_rows(), trace

    def optimise(self, x0, options=None):
        """DeviceSCG over the whole batch in lock step: (x (B, len_x), f (B,), statistics)."""
        from .scg import DeviceSCG
        opt = DeviceSCG(self._context(), *(() if options is None else (options,)))
        x, f = opt(self._stack(x0))
        self._x = np.asarray(x, dtype=float).reshape(self.B, self.len_x)
        self._f = np.atleast_1d(np.asarray(f, dtype=float))
        return self._x, self._f, opt.statistics

    def _outputs_at(self, x):
        """F and the output arrays of every problem at x: one evaluation and one download per x, shared by the B result(k) calls."""
        ctx = self._context()
        c = self._outputs
        if c is not None and c[0] == self._ctx_key and np.array_equal(c[1], x):
            return c[2], c[3]
        f = self.free_energy(x)
        arrays = {}
        for key in ("mt", "st", "Efx", "Edf", "lamt", "psit"):
            val = np.asarray(ctx.fetch(key))
            arrays[key] = val[None] if self.B == 1 else val
        self._outputs = (self._ctx_key, x.copy(), f, arrays)
        return f, arrays

    def result(self, k, x=None, fx=None):
        """Problem k's result dictionary in the form save_results writes (fx, at, bt, m0, s0, mt, st, lamt, psit, Efx, Edf),
        at x (B, len_x) or, by default, at the point the last optimise() returned."""
        if x is None:
            if self._x is None:
                raise RuntimeError(" ProblemBatch.result: no optimisation has run; pass x.")
            x, fx = self._x, self._f
        x = self._stack(x)
        f, arrays = self._outputs_at(x)
        vgp = self.vgps[k]
        n, d = self.dim_n, self.dim_d
        xk = x[k]
        out = {"fx": float(f[k]) if fx is None else float(np.asarray(fx).ravel()[k])}
        if vgp.model.single_dim:
            out["at"], out["bt"] = xk[:n], xk[n:]
        else:
            out["at"], out["bt"] = xk[:n * d * d].reshape(n, d, d), xk[n * d * d:].reshape(n, d)
        out["m0"], out["s0"] = vgp.output["m0"], vgp.output["s0"]
        for key, arr in arrays.items():
            val = arr[k].copy()
            if vgp.model.single_dim:
                val = val.reshape(n)
            out[key] = val
        return out
