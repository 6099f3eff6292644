"""
tests/extended_ref.py -- TEST INFRASTRUCTURE: the Lorenz-96 energy of oracle/vgpa_oracle.py in np.longdouble (x87 80-bit, 64-bit
mantissa), and the seeded covariance generators of the conditioning / not-positive-definite tests.

Why: the fp64 oracle factors S_t with LAPACK, so against an ill-conditioned S_t its own rounding (cond * 1e-16) is as large as a
kernel's.  An evaluation with 11 more bits tells the two apart: every test states the kernel's error AND the oracle's against it.

What is restated (same formulas, same quirks, names as in the oracle): _l96_point_lean -> l96_point (Cholesky of (D + kappa) S_t,
sigma points, the drift with its FLATTENED np.roll -- Q1 --, e_t, dEsde_dm, dEsde_dS), l96_mean_drift, l96_mean_jacobian, my_trapz,
energy_l96 (lean), solve_fwd.  np.linalg has no extended precision: the Cholesky factor and its inverse are written out here, one
row-vectorised step per column / row.  Like the oracle, a non-positive pivot raises LinAlgError.

Every input is taken as the fp64 number it is (the conversion to longdouble is exact); nothing is rounded back before the caller
does it.
"""
import numpy as np

LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=LD)


# --------------------------------------------------------------------------- #
#  Linear algebra
# --------------------------------------------------------------------------- #
def cholesky(s):
    """Lower factor of a symmetric matrix (the lower triangle is read), left-looking, one column per step."""
    s = _ld(s)
    d = s.shape[0]
    low = np.zeros((d, d), dtype=LD)
    for j in range(d):
        col = s[j:, j] - low[j:, :j].dot(low[j, :j])
        if not col[0] > 0:
            raise np.linalg.LinAlgError(f"Matrix is not positive definite (pivot {j})")
        low[j, j] = np.sqrt(col[0])
        low[j + 1:, j] = col[1:] / low[j, j]
    return low


def tri_inverse(low):
    """Inverse of a lower-triangular matrix by forward substitution, one row of the inverse per step."""
    low = _ld(low)
    d = low.shape[0]
    inv = np.zeros((d, d), dtype=LD)
    for i in range(d):
        row = -low[i, :i].dot(inv[:i, :])
        row[i] += 1
        inv[i] = row / low[i, i]
    return inv


def spd_inverse(s):
    linv = tri_inverse(cholesky(s))
    return linv.T.dot(linv)


# --------------------------------------------------------------------------- #
#  The Lorenz-96 energy (oracle: l96_drift, l96_mean_drift, l96_mean_jacobian, _l96_point_lean, my_trapz, energy_l96)
# --------------------------------------------------------------------------- #
def l96_drift(x, theta):
    return (np.roll(x, -1) - np.roll(x, +2)) * np.roll(x, +1) - x + theta           # no axis: the flat roll (Q1)


def l96_mean_drift(mt, st, theta):
    idx = np.arange(mt.size)
    f1, b1, b2 = np.roll(idx, -1), np.roll(idx, +1), np.roll(idx, +2)
    return st[f1, b1] - st[b2, b1] + (np.roll(mt, -1) - np.roll(mt, +2)) * np.roll(mt, +1) - mt + theta


def l96_mean_jacobian(x):
    d = x.size
    idx = np.arange(d)
    f1i, b1i, b2i = np.roll(idx, -1), np.roll(idx, +1), np.roll(idx, +2)
    f1x, b1x, b2x = np.roll(x, -1), np.roll(x, +1), np.roll(x, +2)
    jac = np.zeros((d, d), dtype=LD)
    for k in range(d):                         # (the oracle's order of assignments: at D = 4 two of the four columns coincide)
        row = np.zeros(d, dtype=LD)
        row[k] = -1
        row[f1i[k]] = b1x[k]
        row[b2i[k]] = -b1x[k]
        row[b1i[k]] = f1x[k] - b2x[k]
        jac[k] = row
    return jac


def l96_point(theta, isg, at, bt, mt, st):
    """One grid point: (m_bar, e_t, dEsde_dm, dEsde_dS, resid_bar) -- resid_bar is the unscented mean of the residual BEFORE
    squaring, whose Sigma^-1-weighted sum is the integrand of dF/dtheta."""
    theta, isg, at, bt, mt, st = _ld(theta), _ld(isg), _ld(at), _ld(bt), _ld(mt), _ld(st)
    d = mt.size
    kappa = LD(np.float64(1.05) * d)           # the fp64 constant of the oracle and the kernels: an input, not a rounding of theirs
    c = d + kappa
    low = cholesky(c * st)
    chi = np.concatenate((mt[np.newaxis, :], mt + low.T, mt - low.T))
    lin = l96_drift(chi, theta) + chi.dot(at.T) - bt
    resid = lin ** 2
    v = resid.dot(isg)
    w0, w = kappa / c, 1 / (2 * c)
    m_bar = w0 * resid[0] + w * np.sum(resid[1:], axis=0)
    e_t = isg.dot(m_bar) / 2
    linv = tri_inverse(low)
    delta = w * (v[1:d + 1] - v[d + 1:])
    e_sum = w * (v[1:d + 1] + v[d + 1:])
    de_dm = c * linv.T.dot(delta) / 2
    de_ds = c * (linv.T * (c * e_sum / 2 - e_t)).dot(linv) / 2
    return m_bar, e_t, de_dm, de_ds, w0 * lin[0] + w * np.sum(lin[1:], axis=0)


def _trapz0(fx, dx):
    return np.sum(dx * (fx[1:] + fx[:-1]) / 2, axis=0)


def my_trapz(fx, dx, obs_t=None):
    fx, dx = _ld(fx), LD(dx)
    if obs_t is None or len(obs_t) == 0:
        return _trapz0(fx, dx)
    total, first = 0, 0
    for k, last in enumerate(obs_t):
        total = total + _trapz0(fx[first:last + 1], dx)
        first = obs_t[k]
    if first != fx.shape[0] - 1:
        total = total + _trapz0(fx[first:], dx)
    return total


def energy_l96(theta, sigma, dt, lin_a, off_b, m, s, obs_t=None):
    """oracle.energy_l96(faithful=False) on Sigma itself (inverted here): a dict of longdouble values under the names of
    Context.energy / the oracle's state -- Esde, e_t, Ef, Edf, dEsde_dm, dEsde_dS, dEsde_dth, dEsde_dsig -- and theta_integral, the
    trapezoid of sum_i (Sigma^-1)_ii resid_bar_i (= dEsde/dtheta of a scalar theta)."""
    lin_a, off_b, m, s = _ld(lin_a), _ld(off_b), _ld(m), _ld(s)
    n, d = m.shape
    inv_sigma = spd_inverse(sigma)
    isg = np.diag(inv_sigma).copy()
    e_t = np.zeros(n, dtype=LD)
    ef, edf = np.zeros((n, d), dtype=LD), np.zeros((n, d, d), dtype=LD)
    de_dm, de_ds = np.zeros((n, d), dtype=LD), np.zeros((n, d, d), dtype=LD)
    dth, dsg, tg = np.zeros((n, d), dtype=LD), np.zeros((n, d), dtype=LD), np.zeros(n, dtype=LD)
    theta = LD(theta)
    for t in range(n):
        ef[t] = l96_mean_drift(m[t], s[t], theta)
        edf[t] = l96_mean_jacobian(m[t])
        dsg[t], e_t[t], de_dm[t], de_ds[t], rbar = l96_point(theta, isg, lin_a[t], off_b[t], m[t], s[t])
        dth[t] = ef[t] + m[t].dot(lin_a[t].T) - off_b[t]
        tg[t] = isg.dot(rbar)
    return dict(Esde=my_trapz(e_t, dt, obs_t), e_t=e_t, Ef=ef, Edf=edf, dEsde_dm=de_dm, dEsde_dS=de_ds,
                dEsde_dth=isg * my_trapz(dth, dt, obs_t),
                dEsde_dsig=-inv_sigma.dot(np.diag(my_trapz(dsg, dt, obs_t))).dot(inv_sigma) / 2,
                theta_integral=my_trapz(tg, dt, obs_t))


def esde_l96(theta, sigma, dt, lin_a, off_b, m, s):
    """E_sde alone (no inverse of the factor): what the central difference in theta needs."""
    lin_a, off_b, m, s = _ld(lin_a), _ld(off_b), _ld(m), _ld(s)
    isg = np.diag(spd_inverse(sigma)).copy()
    theta = LD(theta)
    d = m.shape[1]
    kappa = LD(np.float64(1.05) * d)
    c = d + kappa
    e_t = np.zeros(m.shape[0], dtype=LD)
    for t in range(m.shape[0]):
        low = cholesky(c * s[t])
        chi = np.concatenate((m[t][np.newaxis, :], m[t] + low.T, m[t] - low.T))
        resid = (l96_drift(chi, theta) + chi.dot(lin_a[t].T) - off_b[t]) ** 2
        e_t[t] = isg.dot(kappa / c * resid[0] + np.sum(resid[1:], axis=0) / (2 * c)) / 2
    return my_trapz(e_t, dt)


def theta_gradient_fd(theta, sigma, dt, lin_a, off_b, m, s, step=0.5):
    """Central difference of the extended E_sde in the scalar theta: E_sde is quadratic in theta, so this is its derivative."""
    step = LD(step)
    up = esde_l96(LD(theta) + step, sigma, dt, lin_a, off_b, m, s)
    dn = esde_l96(LD(theta) - step, sigma, dt, lin_a, off_b, m, s)
    return (up - dn) / (2 * step)


def solve_fwd(method, dt, lin_a, off_b, m0, s0, sigma):
    """oracle.solve_fwd (n-D models) in longdouble, Q2 of the RK2 predictor included."""
    lin_a, off_b, sigma, dt = _ld(lin_a), _ld(off_b), _ld(sigma), LD(dt)
    n, d = off_b.shape
    mt, st = np.zeros((n, d), dtype=LD), np.zeros((n, d, d), dtype=LD)
    mt[0], st[0] = _ld(m0), _ld(s0)
    h = dt / 2

    def f_m(m, a, b):
        return -a.dot(m) + b

    def f_s(s, a):
        return -a.dot(s) - s.dot(a.T) + sigma

    for k in range(n - 1):
        ak, bk, mk, sk = lin_a[k], off_b[k], mt[k], st[k]
        ap, bp = lin_a[k + 1], off_b[k + 1]
        am, bm = (ak + ap) / 2, (bk + bp) / 2
        if method == "euler":
            mt[k + 1] = mk + f_m(mk, ak, bk) * dt
            st[k + 1] = sk + f_s(sk, ak) * dt
        elif method == "heun":
            p = f_m(mk, ak, bk)
            mt[k + 1] = mk + h * (p + f_m(mk + p * dt, ap, bp))
            p = f_s(sk, ak)
            st[k + 1] = sk + h * (p + f_s(sk + p * dt, ap))
        elif method == "rk2":
            mt[k + 1] = mk + dt * f_m(mk + h * f_m(mk, ak, bk), am, bm)
            st[k + 1] = sk + dt * f_s(sk + h * f_s(sk, sk), am)
        elif method == "rk4":
            k1 = f_m(mk, ak, bk)
            k2 = f_m(mk + h * k1, am, bm)
            k3 = f_m(mk + h * k2, am, bm)
            k4 = f_m(mk + dt * k3, ap, bp)
            mt[k + 1] = mk + dt * (k1 + 2 * (k2 + k3) + k4) / 6
            l1 = f_s(sk, ak)
            l2 = f_s(sk + h * l1, am)
            l3 = f_s(sk + h * l2, am)
            l4 = f_s(sk + dt * l3, ap)
            st[k + 1] = sk + dt * (l1 + 2 * (l2 + l3) + l4) / 6
        else:
            raise ValueError(f"unknown integration method: {method}")
    return mt, st


# --------------------------------------------------------------------------- #
#  Seeded inputs
# --------------------------------------------------------------------------- #
def haar(rng, d):
    """An orthogonal matrix from the Haar measure: QR of a Gaussian matrix with the signs of R's diagonal fixed."""
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def spd_with_spectrum(rng, d, cond, top=0.05):
    """Q diag(lambda) Q^T, Q Haar, lambda log-spaced from `top` down to top / cond; exactly symmetric."""
    lam = top * np.logspace(0.0, -np.log10(cond), d) if d > 1 else np.array([top])
    q = haar(rng, d)
    s = (q * lam).dot(q.T)
    return (s + s.T) / 2.0


def break_at_pivot(s, j):
    """S - (1 + 1e-3) L[j,j]^2 e_j e_j^T for the factor L of the SPD S: the pivots before j are untouched (they never read entry
    (j, j)) and pivot j becomes -1e-3 L[j,j]^2 -- the first to fail, by a margin that is no rounding error."""
    s = np.array(s, dtype=float)
    low = cholesky(s)
    s[j, j] -= float((1 + LD(1) / 1000) * low[j, j] ** 2)
    return s
