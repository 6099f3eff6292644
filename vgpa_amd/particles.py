"""
ParticleFilterResult: one problem's record of the guided particle filter (vgpa_particle_filter).

The posterior process is the proposal.  Its draws are weighted against the model SDE and the data as in weights.PathWeights, but the
weights are taken in observation by observation, and the cloud of n particles is resampled (systematic resampling) whenever its effective
sample size drops below ess_fraction n.  Resampling preserves the mean weight, so log_evidence() is the formula of PathWeights: with
ess_fraction = 0 the record holds exactly the weights of importance_weights(); with resampling the estimate stays unbiased and its variance
grows linearly, not exponentially, with the number of observations.  Resampling couples the particles of a problem: from the first
resampling on, particle i depends on n (the prefix property of sample_paths ends there).
"""
import numpy as np

__all__ = ["ParticleFilterResult"]


class ParticleFilterResult(object):
    """log_w (n,): the final unnormalised log-weights; state (n, D): the final particles; over the problem's M_p observations: ess (M_p,),
    resampled (M_p,) bool, and -- history=True, else None -- ancestors (M_p, n): slot i behind observation j came from slot ancestors[j, i]
    of clouds[j] (the identity where the cloud was carried on), clouds (M_p, n, D): the particles at observation j before the resampling
    decision.  The 1-D models drop the last axis of state and clouds."""

    def __init__(self, log_w, state, ess, resampled, ancestors=None, clouds=None) -> None:
        self.log_w = np.asarray(log_w, dtype=float).ravel()
        if self.log_w.size < 1:
            raise ValueError(" ParticleFilterResult: at least one particle.")
        self.state = np.asarray(state, dtype=float)
        self.ess = np.asarray(ess, dtype=float).ravel()
        self.resampled = np.asarray(resampled).astype(bool).ravel()
        self.ancestors = None if ancestors is None else np.asarray(ancestors, dtype=np.int64)
        self.clouds = None if clouds is None else np.asarray(clouds, dtype=float)
        if self.state.shape[0] != self.log_w.size or self.ess.size != self.resampled.size:
            raise ValueError(" ParticleFilterResult: log_w, state, ess and resampled do not belong together.")
        if self.ancestors is not None and self.ancestors.shape != (self.ess.size, self.log_w.size):
            raise ValueError(" ParticleFilterResult: ancestors must be (observations, particles).")

    def __len__(self):
        return self.log_w.size

    def _normalised(self):
        w = np.exp(self.log_w - np.max(self.log_w))
        return w / np.sum(w)

    def log_evidence(self):
        """logsumexp(log_w) - log n: the estimate of log p(y | theta, Sigma), unbiased in the evidence with or without resampling"""
        top = np.max(self.log_w)
        return float(top + np.log(np.sum(np.exp(self.log_w - top))) - np.log(self.log_w.size))

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
