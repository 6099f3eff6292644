"""
PathWeights: the importance weights of sampled posterior paths against the model SDE and the data (vgpa_sample_paths_weighted).

    log w = init + path + obs
      path   the log-ratio of the discrete path densities, model SDE over posterior process (summed on the device, step by step)
      obs    the Gaussian log-likelihood of the observations along the path (summed on the device)
      init   log N(x_0; mu0, tau0) - log N(x_0; m0, S0), computed on the host from every path's x_0 (0 for a given start)

The paths are draws of the variational approximation; the weights say how far it is from the smoothing distribution of the data, and make
the draws usable as a proposal: log_evidence() estimates log p(y | theta, Sigma), ess() is the effective sample size, mean() and
resample() give asymptotically exact smoothing expectations.  These are true Gaussian densities, not the reference's energy terms:
-mean(log_w) is NOT the free energy F.
"""
import numpy as np

__all__ = ["PathWeights", "gauss_logpdf", "init_term"]


def gauss_logpdf(x, mean, cov):
    """log N(x; mean, cov) of every row of x (n, D); cov (D, D), or a scalar variance with x (n,) / (n, 1)."""
    x = np.asarray(x, dtype=float)
    x = x.reshape(x.shape[0], -1)
    d = x.shape[1]
    cov = np.asarray(cov, dtype=float).reshape(d, d)
    z = x - np.asarray(mean, dtype=float).reshape(1, d)
    fac = np.linalg.cholesky(cov)
    u = np.linalg.solve(fac, z.T)
    return -0.5 * np.sum(u * u, axis=0) - np.sum(np.log(fac.diagonal())) - 0.5 * d * np.log(2.0 * np.pi)


def init_term(start, mu0, tau0, m0, s0):
    """log N(x_0; mu0, tau0) - log N(x_0; m0, S0) of every x_0 in start (n, D): the prior of the model over the start the paths were drawn from"""
    return gauss_logpdf(start, mu0, tau0) - gauss_logpdf(start, m0, s0)


class PathWeights(object):
    """init, path, obs: (n,) each; log_w their sum; paths: (n, n_keep, D) ((n, n_keep) for the 1-D models) or None."""

    def __init__(self, init, path, obs, paths=None) -> None:
        self.init, self.path, self.obs = (np.asarray(v, dtype=float).ravel() for v in (init, path, obs))
        if not (self.init.size == self.path.size == self.obs.size and self.path.size >= 1):
            raise ValueError(" PathWeights: init, path and obs must have the same length >= 1.")
        self.log_w = self.init + self.path + self.obs
        self.paths = paths

    def __len__(self):
        return self.log_w.size

    def _normalised(self):
        w = np.exp(self.log_w - np.max(self.log_w))
        return w / np.sum(w)

    def log_evidence(self):
        """log (1/n) sum_i w_i: the importance-sampling estimate of log p(y | theta, Sigma), shifted by max log w (finite for log w ~ -700)"""
        top = np.max(self.log_w)
        return float(top + np.log(np.sum(np.exp(self.log_w - top))) - np.log(self.log_w.size))

    def ess(self):
        """(sum w)^2 / sum w^2, between 1 and n"""
        w = np.exp(self.log_w - np.max(self.log_w))      # (unnormalised: equal weights give n exactly)
        return float(np.sum(w) ** 2 / np.sum(w * w))

    def resample(self, seed):
        """Systematic resampling: n indices, path i about n w_i / sum w times; one uniform from `seed`."""
        n = self.log_w.size
        u = (np.random.default_rng(seed).random() + np.arange(n)) / n
        cum = np.cumsum(self._normalised())
        cum[-1] = 1.0
        return np.searchsorted(cum, u, side="right").clip(0, n - 1)

    def mean(self, values):
        """The self-normalised weighted mean sum_i w_i values_i / sum_i w_i over the leading axis of values (n, ...)."""
        values = np.asarray(values, dtype=float)
        return np.tensordot(self._normalised(), values, axes=(0, 0))
