"""
The two-time covariance of the posterior process as Context.lag_covariance returns it (vgpa_lag_covariance):
K(k, s) = Cov[x_k, x_s] = Phi(k, s) S_s for grid indices k >= s, from a set of anchors s to the end of the grid -- or the propagator
Phi(k, s) itself.  Host-side bookkeeping only: which block is where, the transpose rule K(k, s) = K(s, k)^T for k < s, and the
quantities made of two times (correlations, the joint covariance over the anchors, the variance of an increment).
"""
import numpy as np


class LagCovariance:
    """values (..., n_anchor, n_keep, D, D): block [a, j] is K(grid[j], anchors[a]) (kind "covariance") or Phi(grid[j], anchors[a]) (kind
    "propagator"), zero where grid[j] < anchors[a].  Leading axes (a batch) are carried through every result.
    anchors (n_anchor,): strictly increasing grid indices;  grid (n_keep,): the kept grid indices 0, stride, 2 stride, ..."""

    def __init__(self, values, anchors, grid, kind="covariance"):
        self.values = np.asarray(values)
        self.anchors = np.asarray(anchors, dtype=np.int64).ravel()
        self.grid = np.asarray(grid, dtype=np.int64).ravel()
        self.kind = str(kind)
        if self.kind not in ("covariance", "propagator"):
            raise ValueError(f" Unknown kind of lag covariance -> {kind}")
        if self.values.ndim < 4 or self.values.shape[-4:-2] != (self.anchors.size, self.grid.size) or self.values.shape[-1] != self.values.shape[-2]:
            raise ValueError(f"values has shape {self.values.shape}, expected (..., {self.anchors.size}, {self.grid.size}, D, D)")
        self._anchor_at = {int(s): a for a, s in enumerate(self.anchors)}
        self._kept_at = {int(k): j for j, k in enumerate(self.grid)}

    def problem(self, p):
        """the record of problem p of a batched result"""
        if self.values.ndim < 5:
            raise IndexError("not a batched result")
        return LagCovariance(self.values[p], self.anchors, self.grid, self.kind)

    def block(self, k, s):
        """values at anchor s and kept grid index k >= s; KeyError where s is no anchor, k is not kept or k < s"""
        k, s = int(k), int(s)
        if s not in self._anchor_at:
            raise KeyError(f"{s} is not an anchor (anchors: {self.anchors.tolist()})")
        if k < s:
            raise KeyError(f"the block of anchor {s} starts at its own grid index ({k} < {s})")
        if k not in self._kept_at:
            raise KeyError(f"grid index {k} is not on the kept grid (stride {int(self.grid[1] - self.grid[0]) if self.grid.size > 1 else 1})")
        return self.values[..., self._anchor_at[s], self._kept_at[k], :, :]

    def cov(self, k, s):
        """K(k, s) = Cov[x_k, x_s], (..., D, D): the block of anchor s for k >= s, the transpose of the block of anchor k for k < s.
        KeyError when the earlier of the two indices is not an anchor (or the later one not kept)."""
        if self.kind != "covariance":
            raise ValueError("cov() needs a result of kind \"covariance\" (this one holds propagators: block(k, s))")
        k, s = int(k), int(s)
        if k >= s and s in self._anchor_at:
            return self.block(k, s)
        if k <= s and k in self._anchor_at:
            return np.swapaxes(self.block(s, k), -1, -2)
        raise KeyError(f"neither {min(k, s)} nor an index before it anchors the pair ({k}, {s}): K(k, s) is computed from the earlier index")

    def marginal(self, k, st=None):
        """S_k, (..., D, D): from st (..., Np, D, D), the marginal covariances on the whole grid, or -- st=None -- from the row k = s of anchor k"""
        k = int(k)
        if st is not None:
            st = np.asarray(st)
            return st[..., k, :, :] if st.ndim >= 3 else st[..., k].reshape(st.shape[:-1] + (1, 1))
        return self.cov(k, k)

    def corr(self, k, s, st=None):
        """Corr[x_k,i, x_s,j] = K_ij / sqrt(S_k,ii S_s,jj), (..., D, D); the marginals as in marginal()"""
        dk = np.sqrt(np.diagonal(self.marginal(k, st), axis1=-2, axis2=-1))
        ds = np.sqrt(np.diagonal(self.marginal(s, st), axis1=-2, axis2=-1))
        return self.cov(k, s) / (dk[..., :, None] * ds[..., None, :])

    def increment_var(self, k, s, st=None):
        """Cov[x_k - x_s] = S_k + S_s - K(k, s) - K(k, s)^T, (..., D, D)"""
        c = self.cov(k, s)
        return self.marginal(k, st) + self.marginal(s, st) - c - np.swapaxes(c, -1, -2)

    def joint(self):
        """The covariance of (x_{s_1}, ..., x_{s_n}) over the anchors, (..., n D, n D), symmetric: block (i, j) is K(s_i, s_j).  Every anchor
        must be on the kept grid (KeyError otherwise)."""
        n, d = self.anchors.size, self.values.shape[-1]
        out = np.empty(self.values.shape[:-4] + (n * d, n * d), dtype=self.values.dtype)
        for i, si in enumerate(self.anchors):
            for j, sj in enumerate(self.anchors[:i + 1]):
                c = self.cov(si, sj)
                out[..., i * d:(i + 1) * d, j * d:(j + 1) * d] = c
                if j < i:
                    out[..., j * d:(j + 1) * d, i * d:(i + 1) * d] = np.swapaxes(c, -1, -2)
        return out
