"""
tests/extended_ref.py -- TEST INFRASTRUCTURE: the sweep of oracle/vgpa_oracle.py (forward and backward steppers, observation terms,
the four models' energies, the gradient assembly) in np.longdouble (x87 80-bit, 64-bit mantissa), the particle half one step or one
reduction at a time (Box-Muller normals from the Philox words, the model drifts and phi, one Euler-Maruyama step, the path / observation
terms and the statistics rows of stored paths, self-normalised weighted sums, the back-propagated stretch weights: each in longdouble or,
as the fp64 yardstick, in float64), and the seeded covariance generators of the conditioning / not-positive-definite tests.

Why: the fp64 oracle factors S_t with LAPACK, so against an ill-conditioned S_t its own rounding (cond * 1e-16) is as large as a
kernel's.  An evaluation with 11 more bits tells the two apart: every test states the kernel's error AND the oracle's against it.

What is restated (same formulas, same quirks, names as in the oracle): _l96_point_lean -> l96_point (Cholesky of (D + kappa) S_t,
sigma points, the drift with its FLATTENED np.roll -- Q1 --, e_t, dEsde_dm, dEsde_dS), l96_mean_drift, l96_mean_jacobian, my_trapz,
energy_l96 (lean), solve_fwd; solve_bwd (zero-padded mid-points, Q3, jumps after the step: Q9), obs_terms (Q4), gradient, energy_ou,
energy_dw (Q7), energy_l63 (with l63_drift_theta: dEsde_dth) and sweep (lean); theta_gradient (dF/dtheta of a problem from the restated
sweep state) and, for the scalar results that sum terms of either sign, their summands (obs_terms(parts=True), the dth_t of the
energies, trapezoid_summands) and kappa = sum |summand| / |sum summand|.  The scalar models run the n-D recursions on 1 x 1 matrices.  np.linalg has no extended precision: the Cholesky factor and its inverse are written out here, one
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
    """oracle.solve_fwd in longdouble, Q2 of the RK2 predictor included.  The scalar models' 1-D arrays (lin_a, off_b of shape (n,),
    scalar m0 / s0 / sigma) run as 1 x 1 matrices -- the same arithmetic -- and come back 1-D."""
    if np.ndim(off_b) == 1:
        mt, st = solve_fwd(method, dt, _ld(lin_a).reshape(-1, 1, 1), _ld(off_b).reshape(-1, 1), _ld(m0).reshape(1), _ld(s0).reshape(1, 1),
                           _ld(sigma).reshape(1, 1))
        return mt[:, 0], st[:, 0, 0]
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


def _mid_padded(z):
    """The mid-points (z[k] + z[k + 1]) / 2, zero-padded back to Np rows (the oracle's _mid_padded)."""
    return np.concatenate(((z[:-1] + z[1:]) / 2, np.zeros((1,) + z.shape[1:], dtype=LD)), axis=0)


def solve_bwd(method, dt, lin_a, de_dm, de_ds, jump_m, jump_s):
    """oracle.solve_bwd in longdouble, all four methods: lam_t with lam.dot(a.T) (Q3), the zero-padded mid-points, the jumps added
    after the step (Q9).  The scalar models' 1-D arrays run as 1 x 1 matrices and come back 1-D."""
    if np.ndim(de_dm) == 1:
        a, es, js = (_ld(v).reshape(-1, 1, 1) for v in (lin_a, de_ds, jump_s))
        lam, psi = solve_bwd(method, dt, a, _ld(de_dm).reshape(-1, 1), es, _ld(jump_m).reshape(-1, 1), js)
        return lam[:, 0], psi[:, 0, 0]
    lin_a, de_dm, de_ds, jump_m, jump_s, dt = _ld(lin_a), _ld(de_dm), _ld(de_ds), _ld(jump_m), _ld(jump_s), LD(dt)
    n, d = de_dm.shape
    lam, psi = np.zeros((n, d), dtype=LD), np.zeros((n, d, d), dtype=LD)
    h = dt / 2

    def f_lam(g, a, lm):
        return -g + lm.dot(a.T)

    def f_psi(g, a, ps):
        return -g + ps.dot(a) + a.T.dot(ps)

    if method in ("rk2", "rk4"):
        a_mid, em_mid, es_mid = _mid_padded(lin_a), _mid_padded(de_dm), _mid_padded(de_ds)
    for t in range(n - 1, 0, -1):
        at, lt, pt = lin_a[t], lam[t], psi[t]
        if method == "euler":
            lam[t - 1] = lt - f_lam(de_dm[t], at, lt) * dt + jump_m[t - 1]
            psi[t - 1] = pt - f_psi(de_ds[t], at, pt) * dt + jump_s[t - 1]
        elif method == "heun":
            ak = lin_a[t - 1]
            p = f_lam(de_dm[t], at, lt)
            lam[t - 1] = lt - h * (p + f_lam(de_dm[t - 1], ak, lt - p * dt)) + jump_m[t - 1]
            p = f_psi(de_ds[t], at, pt)
            psi[t - 1] = pt - h * (p + f_psi(de_ds[t - 1], ak, pt - p * dt)) + jump_s[t - 1]
        elif method == "rk2":
            ak, em, es = a_mid[t - 1], em_mid[t - 1], es_mid[t - 1]
            lam[t - 1] = lt - dt * f_lam(em, ak, lt - h * f_lam(de_dm[t], at, lt)) + jump_m[t - 1]
            psi[t - 1] = pt - dt * f_psi(es, ak, pt - h * f_psi(de_ds[t], at, pt)) + jump_s[t - 1]
        elif method == "rk4":
            ak, em, es = a_mid[t - 1], em_mid[t - 1], es_mid[t - 1]
            k1 = f_lam(de_dm[t], at, lt)
            k2 = f_lam(em, ak, lt - h * k1)
            k3 = f_lam(em, ak, lt - h * k2)
            k4 = f_lam(de_dm[t - 1], lin_a[t - 1], lt - dt * k3)
            lam[t - 1] = lt - dt * (k1 + 2 * (k2 + k3) + k4) / 6 + jump_m[t - 1]
            l1 = f_psi(de_ds[t], at, pt)
            l2 = f_psi(es, ak, pt - h * l1)
            l3 = f_psi(es, ak, pt - h * l2)
            l4 = f_psi(de_ds[t - 1], lin_a[t - 1], pt - dt * l3)
            psi[t - 1] = pt - dt * (l1 + 2 * (l2 + l3) + l4) / 6 + jump_s[t - 1]
        else:
            raise ValueError(f"unknown integration method: {method}")
    return lam, psi


# --------------------------------------------------------------------------- #
#  Observation terms (oracle: eobs, eobs_gradients)
# --------------------------------------------------------------------------- #
LOG2PI = LD(np.float64(np.log(2.0 * np.pi)))        # the oracle's fp64 constant: an input, like kappa


def obs_terms(p, mt, st, parts=False, q4=True):
    """(E_obs, jump_m, jump_s) of oracle.eobs / eobs_gradients: dense R and a non-identity H through cholesky / tri_inverse; the
    covariance diagonal is indexed by the observation COUNTER, as the oracle does (Q4; q4=False: by the observation's grid index, which
    neither the oracle nor a kernel does -- for the tests that show the difference).  parts=True: a fourth member, the dict
    (terms (M,), const) with E_obs = sum(terms) + const -- the per-observation summands and the normalisation constant, for kappa."""
    mt, st = _ld(mt), _ld(st)
    obs_t = np.asarray(p.obs_t, dtype=np.int64)
    obs_y, r = _ld(p.obs_y), _ld(p.obs_noise)
    if p.single_dim:
        ex2 = mt[obs_t] ** 2 + st[obs_t]
        const = obs_t.size * (LOG2PI + np.log(r)) / 2
        e_obs = np.sum(obs_y ** 2 - 2 * obs_y * mt[obs_t] + ex2) / 2 / r + const
        h = LD(1) if p.obs_h is None else _ld(p.obs_h)
        jm, js = np.zeros(mt.shape[0], dtype=LD), np.zeros(mt.shape[0], dtype=LD)
        jm[obs_t] = -(obs_y - h * mt[obs_t]) / r
        js[obs_t] = 1 / (2 * r)
        if parts:
            return e_obs, jm, js, dict(terms=(obs_y ** 2 - 2 * obs_y * mt[obs_t] + ex2) / 2 / r, const=const)
        return e_obs, jm, js
    n, d = mt.shape
    dim_m, dim_o = obs_y.shape
    h = np.eye(dim_o, dtype=LD) if p.obs_h is None else _ld(p.obs_h)
    w = (obs_y - mt[obs_t]).dot(h)
    low = cholesky(r)
    inv_c = tri_inverse(low)
    inv_r = inv_c.T.dot(inv_c)
    z = w.dot(inv_c.T)
    acc, terms = LD(0), np.zeros(dim_m, dtype=LD)
    for k in range(dim_m):
        fit, var = z[k].dot(z[k]), np.diag(inv_r).dot(np.diag(st[k if q4 else obs_t[k]]))   # Q4: st[k], not st[obs_t[k]]
        acc = acc + fit + var                                                              # (the oracle's order of additions)
        terms[k] = fit + var
    log_det_r = 2 * np.sum(np.log(np.diag(low)))
    e_obs = (acc + dim_m * (dim_o * LOG2PI + log_det_r)) / 2
    jm, js = np.zeros((n, d), dtype=LD), np.zeros((n, d, d), dtype=LD)
    for k, tn in enumerate(obs_t):
        jm[tn] = -h.T.dot(inv_r).dot(w[k])
        js[tn] = h.T.dot(inv_r).dot(h) / 2
    if parts:
        return e_obs, jm, js, dict(terms=terms / 2, const=dim_m * (dim_o * LOG2PI + log_det_r) / 2)
    return e_obs, jm, js


def kappa(summands, axis=None):
    """sum |summand| / |sum summand| of a sum of terms of either sign: by how much its relative rounding error may exceed the unit
    roundoff whatever the order of the additions (1 for terms of one sign; inf for a sum that is exactly zero)."""
    summands = _ld(summands)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.sum(np.abs(summands), axis=axis) / np.abs(np.sum(summands, axis=axis))
    return float(k) if np.ndim(k) == 0 else np.asarray(k, dtype=float)


def trapezoid_summands(fx, dx):
    """The values of fx (time along axis 0) times their trapezoid weights: dx inside, dx / 2 at both ends -- sum(axis=0) is my_trapz, whose
    pieces between observations add up to the one global rule."""
    w = np.full(np.shape(fx)[0], LD(dx), dtype=LD)
    w[0], w[-1] = w[0] / 2, w[-1] / 2
    return _ld(fx) * w.reshape((-1,) + (1,) * (np.ndim(fx) - 1))


# --------------------------------------------------------------------------- #
#  The energies of the other three models (oracle: gm, gm_dm, gm_ds, energy_ou, energy_dw, l63_point, energy_l63)
# --------------------------------------------------------------------------- #
def gm(m, v, order):
    return {2: lambda: m ** 2 + v, 3: lambda: m ** 3 + 3 * m * v, 4: lambda: m ** 4 + 6 * m ** 2 * v + 3 * v ** 2,
            6: lambda: m ** 6 + 15 * m ** 4 * v + 45 * m ** 2 * v ** 2 + 15 * v ** 3}[order]()


def gm_dm(m, v, order):
    return {2: lambda: 2 * m, 3: lambda: 3 * (m ** 2 + v), 4: lambda: 4 * (m ** 3 + 3 * m * v),
            6: lambda: 6 * (m ** 5 + 10 * m ** 3 * v + 15 * m * v ** 2)}[order]()


def gm_ds(m, v, order):
    return {2: lambda: np.ones(np.shape(m), dtype=LD), 3: lambda: 3 * m, 4: lambda: 6 * (m ** 2 + v),
            6: lambda: 15 * m ** 4 + 90 * m ** 2 * v + 45 * v ** 2}[order]()


def energy_ou(theta, sigma, dt, a, b, m, s, obs_t=None):
    """oracle.energy_ou: a dict under the names of energy_l96."""
    theta, sigma, a, b, m, s = LD(theta), LD(sigma), _ld(a), _ld(b), _ld(m), _ld(s)
    ex2 = gm(m, s, 2)
    q1 = (theta - a) ** 2
    var_q = ex2 * q1 + 2 * m * (theta - a) * b + b ** 2
    esde = my_trapz(var_q, dt, obs_t) / 2 / sigma
    return dict(Esde=esde, Ef=-theta * m, Edf=-theta * np.ones(m.shape, dtype=LD),
                dEsde_dm=(m * (theta - a) ** 2 + theta * b - a * b) / sigma, dEsde_dS=q1 / 2 / sigma,
                dEsde_dth=my_trapz(ex2 * (theta - a) + m * b, dt, obs_t) / sigma, dEsde_dsig=-esde / sigma,
                dth_t=(ex2 * (theta - a) + m * b) / sigma)


def energy_dw(theta, sigma, dt, a, b, m, s, obs_t=None):
    """oracle.energy_dw (Q7: 8 Ex6 in the energy, 16 Dm6 in its gradient): a dict under the names of energy_l96."""
    theta, sigma, a, b, m, s = LD(theta), LD(sigma), _ld(a), _ld(b), _ld(m), _ld(s)
    c = 4 * theta + a
    c2 = c ** 2
    ex2, ex3, ex4, ex6 = gm(m, s, 2), gm(m, s, 3), gm(m, s, 4), gm(m, s, 6)
    var_q = 8 * (ex6 - c * ex4 + b * ex3) + c2 * ex2 - 2 * b * c * m + b ** 2
    esde = my_trapz(var_q, dt, obs_t) / 2 / sigma
    de_dm = (16 * gm_dm(m, s, 6) - 8 * c * gm_dm(m, s, 4) + 8 * b * gm_dm(m, s, 3) + c2 * gm_dm(m, s, 2) - 2 * b * c) / 2 / sigma
    de_ds = (16 * gm_ds(m, s, 6) - 8 * c * gm_ds(m, s, 4) + 8 * b * gm_ds(m, s, 3) + c2 * gm_ds(m, s, 2)) / 2 / sigma
    return dict(Esde=esde, Ef=4 * (theta * m - ex3), Edf=4 * (theta - 3 * ex2), dEsde_dm=de_dm, dEsde_dS=de_ds,
                dEsde_dth=4 * my_trapz(c * ex2 - 4 * ex4 - b * m, dt, obs_t) / sigma, dEsde_dsig=-esde / sigma,
                dth_t=4 * (c * ex2 - 4 * ex4 - b * m) / sigma)


def l63_point(theta, at, bt, mt, st, isg):
    """oracle.l63_point on longdouble operands.  Its closed-form moments are written with Python operators and constants that are
    exact in both formats (0.5, 2, 4.0), so the oracle's own text evaluates them in the precision of its arguments: every operand is
    converted here, and the result is asserted to be longdouble."""
    from oracle import vgpa_oracle as vo
    efg, de_dm, de_ds = vo.l63_point(_ld(theta), _ld(at), _ld(bt), _ld(mt), _ld(st), _ld(isg))
    assert efg.dtype == de_dm.dtype == de_ds.dtype == LD
    return efg, de_dm, de_ds


def l63_drift_theta(theta, at, bt, mt, st):
    """oracle.l63_drift_theta on longdouble operands, by the route of l63_point: its text has only Python operators and integer constants,
    so it evaluates in the precision of its arguments (asserted)."""
    from oracle import vgpa_oracle as vo
    v = vo.l63_drift_theta(_ld(theta), _ld(at), _ld(bt), _ld(mt), _ld(st))
    assert v.dtype == LD
    return v


def energy_l63(theta, sigma, dt, lin_a, off_b, m, s, obs_t=None):
    """oracle.energy_l63 on Sigma itself (inverted here): a dict under the names of energy_l96; dth_t is the integrand of dEsde_dth
    (Sigma^-1's diagonal folded in), as in energy_ou / energy_dw."""
    theta, lin_a, off_b, m, s = _ld(theta), _ld(lin_a), _ld(off_b), _ld(m), _ld(s)
    n = m.shape[0]
    inv_sigma = spd_inverse(sigma)
    isg = np.diag(inv_sigma).copy()
    e_t = np.zeros(n, dtype=LD)
    ef, edf = np.zeros((n, 3), dtype=LD), np.zeros((n, 3, 3), dtype=LD)
    de_dm, de_ds, dsg = np.zeros((n, 3), dtype=LD), np.zeros((n, 3, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    dth = np.zeros((n, 3), dtype=LD)
    v_s, v_r, v_b = theta
    for t in range(n):
        mt, st = m[t], s[t]
        dsg[t], de_dm[t], de_ds[t] = l63_point(theta, lin_a[t], off_b[t], mt, st, isg)
        e_t[t] = isg.dot(dsg[t]) / 2
        dth[t] = l63_drift_theta(theta, lin_a[t], off_b[t], mt, st)
        ef[t] = (v_s * (mt[1] - mt[0]), v_r * mt[0] - mt[1] - st[2, 0] - mt[0] * mt[2], st[1, 0] + mt[0] * mt[1] - v_b * mt[2])
        edf[t] = ((-v_s, v_s, 0), (v_r - mt[2], -1, -mt[0]), (mt[1], mt[0], -v_b))
    return dict(Esde=my_trapz(e_t, dt, obs_t), e_t=e_t, Ef=ef, Edf=edf, dEsde_dm=de_dm, dEsde_dS=de_ds,
                dEsde_dth=isg * my_trapz(dth, dt, obs_t), dth_t=isg * dth,
                dEsde_dsig=-inv_sigma.dot(np.diag(my_trapz(dsg, dt, obs_t))).dot(inv_sigma) / 2)


def model_energy(p, lin_a, off_b, m, s):
    """oracle.model_energy (lean): the dict of the model's energy."""
    obs_t = list(p.obs_t)
    fn = {"OU": energy_ou, "DW": energy_dw, "L63": energy_l63, "L96": energy_l96}[p.model]
    return fn(p.theta, p.sigma, p.dt, lin_a, off_b, m, s, obs_t)


def theta_gradient(p, x, state):
    """dF/dtheta at fixed (A_t, b_t) from the restated sweep state (mt, st): (value (n_theta,), kappa (n_theta,)).  OU / double well /
    Lorenz-63: the restated dEsde_dth (the reference's member IS dF/dtheta for these models), kappa over its trapezoid-weighted integrand
    values.  Lorenz-96: theta_gradient_fd -- the derivative of the unscented E_sde, which the reference's member is not --, kappa over
    the trapezoid-weighted unscented mean residual, whose integral the same number is."""
    lin_a, off_b = p.split(np.asarray(x))
    if p.model == "L96":
        lin_a, off_b, m, s = _ld(lin_a), _ld(off_b), _ld(state["mt"]), _ld(state["st"])
        isg = np.diag(spd_inverse(p.sigma)).copy()
        tg = np.array([isg.dot(l96_point(p.theta, isg, lin_a[t], off_b[t], m[t], s[t])[4]) for t in range(p.n_pts)], dtype=LD)
        val = theta_gradient_fd(p.theta, p.sigma, p.dt, lin_a, off_b, m, s)
        return np.atleast_1d(val), np.atleast_1d(kappa(trapezoid_summands(tg, p.dt), axis=0))
    en = model_energy(p, lin_a, off_b, state["mt"], state["st"])
    return np.atleast_1d(en["dEsde_dth"]), np.atleast_1d(kappa(trapezoid_summands(en["dth_t"], p.dt), axis=0))


# --------------------------------------------------------------------------- #
#  The gradient assembly and the whole sweep (oracle: gradient, free_energy, sweep)
# --------------------------------------------------------------------------- #
def gradient(p, x, state):
    """oracle.gradient from a longdouble state: (gLa, gLb), each flattened and multiplied by dt; n-D and scalar forms."""
    lin_a, off_b = (_ld(v) for v in p.split(np.asarray(x)))
    n, dt = p.n_pts, LD(p.dt)
    mt, st, lam, psi, efx, edf = (_ld(state[k]) for k in ("mt", "st", "lamt", "psit", "Efx", "Edf"))
    if p.single_dim:
        inv_sigma = 1 / LD(p.sigma)
        db = inv_sigma * (-efx - lin_a * mt + off_b)
        da = inv_sigma * (edf + lin_a) * st - db * mt
        return dt * (da - lam * mt - 2 * psi * st), dt * (db + lam)
    d = p.dim_d
    inv_sigma = spd_inverse(p.sigma)
    gla, glb = np.zeros((n, d, d), dtype=LD), np.zeros((n, d), dtype=LD)
    for k in range(n):
        db = inv_sigma.dot(-efx[k] - lin_a[k].dot(mt[k]) + off_b[k])
        da = inv_sigma.dot(edf[k] + lin_a[k]).dot(st[k]) - np.outer(db, mt[k])
        gla[k] = da - np.outer(lam[k], mt[k]) - 2 * psi[k].dot(st[k])
        glb[k] = db + lam[k]
    return (dt * gla).ravel(), (dt * glb).ravel()


def sweep(p, x, e0):
    """oracle.sweep(p, x, faithful=False) in longdouble: (F, gLa, gLb, state), the state under the oracle's names.  e0 is the float the
    context is given (the prior term is a constant of the problem, not of x): an input, not restated."""
    lin_a, off_b = p.split(np.asarray(x))
    mt, st = solve_fwd(p.method, p.dt, lin_a, off_b, p.m0, p.s0, p.sigma)
    e_obs, jm, js = obs_terms(p, mt, st)
    en = model_energy(p, lin_a, off_b, mt, st)
    lam, psi = solve_bwd(p.method, p.dt, lin_a, en["dEsde_dm"], en["dEsde_dS"], jm, js)
    state = dict(mt=mt, st=st, Efx=en["Ef"], Edf=en["Edf"], lamt=lam, psit=psi, Esde=en["Esde"], Eobs=e_obs, E0=LD(e0),
                 dEsde_dm=en["dEsde_dm"], dEsde_ds=en["dEsde_dS"], dEobs_dm=jm, dEobs_ds=js)
    gla, glb = gradient(p, x, state)
    return LD(e0) + en["Esde"] + e_obs, gla, glb, state


# --------------------------------------------------------------------------- #
#  The particle half (vgpa_amd/csrc/sample.hip): normals, drifts, one Euler-Maruyama step, the sums over stored paths, weighted sums
# --------------------------------------------------------------------------- #
# Every function takes the number type T it computes in: np.longdouble (the reference) or np.float64 (the "oracle": the same text,
# rounded as a careful fp64 evaluation rounds).  Inputs are the fp64 numbers they are; no result is rounded back.
def levels(n):
    """ceil(log2 n): the additions every term of a sum of n terms passes when the sum is added as a balanced tree (0 for n <= 1)"""
    return int(np.ceil(np.log2(n))) if n > 1 else 0


def _sum(a, axis):
    """The sum along `axis` added as a balanced tree (the upper half onto the lower, zero-padded to a power of two): every term passes
    levels(n) additions, each rounded at no more than the sum of the terms' sizes -- the accumulation term of the floors below.  (np.sum
    along an axis that is not the last adds one term at a time: no careful evaluation of a sum of hundreds of terms.)"""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    if n == 0:
        return np.zeros(a.shape[1:], dtype=a.dtype)
    full = 1 << levels(n)
    if full > n:
        a = np.concatenate((a, np.zeros((full - n,) + a.shape[1:], dtype=a.dtype)))
    while a.shape[0] > 1:
        h = a.shape[0] // 2
        a = a[:h] + a[h:]
    return a[0]


def two_pi(T=LD):
    return T(2.0 * np.pi) if T is np.float64 else 8 * np.arctan(LD(1))


def uniforms(seed, k, word, problem, d):
    """(u1, u2), each (..., ceil(d / 2)): the fp64 uniforms of the Philox counter (k, word, problem, pair) under key `seed`.  Integer
    arithmetic and exact conversions only (test_sample_paths_cpu.philox4x32_10 / unit_open): inputs of the normals, not roundings."""
    from test_sample_paths_cpu import philox4x32_10, unit_open
    k, word = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(word, dtype=np.uint64))
    j = np.arange((d + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((k[..., None], word[..., None], np.uint64(problem), j), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return unit_open(r[0], r[1]), unit_open(r[2], r[3])


def box_muller(u1, u2, T=LD, angle=None):
    """(rho cos(2 pi u2), rho sin(2 pi u2), rho) with rho = sqrt(-2 ln u1); angle: the constant in 2 pi's place (a mutant's)"""
    u1, u2 = np.asarray(u1, dtype=T), np.asarray(u2, dtype=T)
    rho = np.sqrt(-2 * np.log(u1))
    ang = (two_pi(T) if angle is None else T(angle)) * u2
    return rho * np.cos(ang), rho * np.sin(ang), rho


def normals(seed, k, word, problem, d, T=LD, angle=None):
    """(xi, rho), each (..., d): the d normals of grid index k drawn with counter word `word` (k, word broadcast), and the radius of each one's pair"""
    u1, u2 = uniforms(seed, k, word, problem, d)
    c, s, rho = box_muller(u1, u2, T, angle)
    z = np.stack((c, s), axis=-1)
    rr = np.stack((rho, rho), axis=-1)
    return z.reshape(z.shape[:-2] + (-1,))[..., :d], rr.reshape(rr.shape[:-2] + (-1,))[..., :d]


def model_drift(model, theta, x, T=LD):
    """(f, sum |monomial|) of the model SDE's drift at x (..., D), in the kernels' grouping of the terms"""
    x, th = np.asarray(x, dtype=T), np.asarray(theta, dtype=T)
    if model == "OU":
        return -th * x, np.abs(th * x)
    if model == "DW":
        return 4 * x * (th - x * x), 4 * np.abs(x * th) + 4 * np.abs(x * x * x)
    if model == "L63":
        x0, x1, x2 = x[..., 0], x[..., 1], x[..., 2]
        f = np.stack((th[0] * (x1 - x0), (th[1] - x2) * x0 - x1, x0 * x1 - th[2] * x2), axis=-1)
        a = np.stack((np.abs(th[0] * x1) + np.abs(th[0] * x0), np.abs(th[1] * x0) + np.abs(x2 * x0) + np.abs(x1),
                      np.abs(x0 * x1) + np.abs(th[2] * x2)), axis=-1)
        return f, a
    assert model == "L96", model
    up, d1, d2 = np.roll(x, -1, axis=-1), np.roll(x, 1, axis=-1), np.roll(x, 2, axis=-1)
    return (up - d2) * d1 - x + th, np.abs(up * d1) + np.abs(d2 * d1) + np.abs(x) + np.abs(th)


def model_phi(model, x, T=LD):
    """phi_j = d f_j / d theta_a(j) at x (..., D): the one parameter component j's drift depends on"""
    x = np.asarray(x, dtype=T)
    if model == "OU":
        return -x
    if model == "DW":
        return 4 * x
    if model == "L63":
        return np.stack((x[..., 1] - x[..., 0], x[..., 0], -x[..., 2]), axis=-1)
    return np.ones(x.shape, dtype=T)


def posterior_drift(lin_a, off_b, x, T=LD):
    """(b - A x, sum_j |A_ij x_j| + |b_i|); lin_a (K, D, D), off_b (K, D) against x (n, K, D), or (D, D), (D,) against (..., D)"""
    a, b, x = np.asarray(lin_a, dtype=T), np.asarray(off_b, dtype=T), np.asarray(x, dtype=T)
    if a.ndim == 3:
        return b - np.einsum("kij,nkj->nki", a, x), np.einsum("kij,nkj->nki", np.abs(a), np.abs(x)) + np.abs(b)
    return b - np.einsum("ij,...j->...i", a, x), np.einsum("ij,...j->...i", np.abs(a), np.abs(x)) + np.abs(b)


def em_step(prev, drift, drift_abs, dt, fac, xi, T=LD, xi_size=None):
    """One Euler-Maruyama step x = (x_prev + dt drift) + R xi with the lower factor R = `fac` (D, D): (x, size), size the number its rounding
    is measured against.  s_i = |x_prev,i| + dt drift_abs_i + sum_j |R_ij xi_j| is the size of the result's terms.  A careful fp64
    evaluation rounds: the first sum at no more than |x_prev,i| + dt drift_abs_i and the second at no more than s_i (together
    2 |x_prev,i| + 2 dt drift_abs_i + n_i); the product dt drift (dt drift_abs_i); the drift's own terms, each once, and their sum, a tree
    of L = levels(D + 1) additions ((1 + L) dt drift_abs_i); the products R_ij xi_j and their sum ((1 + L) n_i, n_i = sum_j |R_ij xi_j|).
    So size_i = 2 |x_prev,i| + (4 + L) dt drift_abs_i + (2 + L) n_i and, xi_size given (the size of each normal's own rounding, in the same
    units), + sum_j |R_ij| xi_size_j: the step takes the xi the device computed, the restatement the xi of the same uniforms in T."""
    prev, fac, xi, dt = np.asarray(prev, dtype=T), np.asarray(fac, dtype=T), np.asarray(xi, dtype=T), T(dt)
    noise = np.einsum("ij,...j->...i", fac, xi)
    new = (prev + dt * np.asarray(drift, dtype=T)) + noise
    lv = levels(prev.shape[-1] + 1)
    size = 2 * np.abs(prev) + (4 + lv) * dt * np.asarray(drift_abs, dtype=T) + (2 + lv) * np.einsum("ij,...j->...i", np.abs(fac), np.abs(xi))
    if xi_size is not None:
        size = size + np.einsum("ij,...j->...i", np.abs(fac), np.asarray(xi_size, dtype=T))
    return new, size


def path_term(model, theta, sigma_diag, dt, lin_a, off_b, stored, T=LD):
    """The path term of stored stride-1 paths (n, Np, D) under a diagonal Sigma: (sum_k inc_k, sum_k |inc_k|, the recovery size), each (n,).
    inc_k = -sum_i d_i (eta_i + dt d_i / 2) / Sigma_ii with d = g - f at x_{k-1} and eta = x_k - (x_{k-1} + dt g), known from the stored
    states up to the two roundings of the state update: recovery = sum_k sum_i |d_i| / Sigma_ii (|x_k,i| + |x_{k-1},i| + dt |g_i|)."""
    x, dt = np.asarray(stored, dtype=T), T(dt)
    isg = 1 / np.asarray(sigma_diag, dtype=T)
    prev, new = x[:, :-1], x[:, 1:]
    g, _ = posterior_drift(np.asarray(lin_a)[:-1], np.asarray(off_b)[:-1], prev, T)
    f, _ = model_drift(model, theta, prev, T)
    d = g - f
    eta = new - (prev + dt * g)
    inc = -np.sum(d * isg * (eta + dt * d / 2), axis=-1)
    rec = np.sum(np.abs(d) * isg * (np.abs(new) + np.abs(prev) + dt * np.abs(g)), axis=(-1, -2))
    return np.sum(inc, axis=-1), np.sum(np.abs(inc), axis=-1), rec


def obs_quadratic(obs_noise, obs_h, d, T=LD):
    """(Q = H R^-1 H^T, log det R) of one problem's observation model"""
    r = np.asarray(obs_noise, dtype=T).reshape(d, d)
    h = np.eye(d, dtype=T) if obs_h is None or d == 1 else np.asarray(obs_h, dtype=T).reshape(d, d)
    if T is np.float64:
        return h @ np.linalg.inv(r) @ h.T, np.linalg.slogdet(r)[1]
    low = cholesky(r)
    linv = tri_inverse(low)
    return h.dot(linv.T.dot(linv)).dot(h.T), 2 * np.sum(np.log(np.diag(low)))


def obs_term(obs_t, obs_y, obs_noise, obs_h, stored, T=LD):
    """The observation term of stored stride-1 paths (n, Np, D): (-sum_n r^T Q r / 2 - const, size), each (n,); const = M (D log 2 pi +
    log det R) / 2 with the fp64 log 2 pi of the library (an input, as in obs_terms).  With q_n = sum_ij |r_i Q_ij r_j| / 2 (the products of
    the form, so that no cancellation inside it hides) size = (5 + 2 levels(D) + levels(M) + cond_2(R)) sum_n |q_n| + 4 |const|: the
    residual y - x is rounded and enters twice (2), the two products of r Q r (2), the D^2 products added as a tree (2 levels(D)), the M
    terms likewise (levels(M)), Q = H R^-1 H^T, whose inverse carries a relative error of cond_2(R) 2^-53 whoever forms it in fp64; the
    constant's logarithm, its sum and its product with M / 2 (3); and the last subtraction, rounded at no more than sum |q_n| + |const|."""
    x = np.asarray(stored, dtype=T)
    d = x.shape[-1]
    obs_t = np.asarray(obs_t, dtype=np.int64).ravel()
    y = np.asarray(obs_y, dtype=T).reshape(obs_t.size, d)
    q, logdet = obs_quadratic(obs_noise, obs_h, d, T)
    const = obs_t.size * (d * T(np.float64(np.log(2.0 * np.pi))) + logdet) / 2
    r = y[None, :, :] - x[:, obs_t, :]
    terms = -np.einsum("nmi,ij,nmj->nm", r, q, r) / 2
    forms = np.einsum("nmi,ij,nmj->nm", np.abs(r), np.abs(q), np.abs(r)) / 2
    cond = T(np.linalg.cond(np.asarray(obs_noise, dtype=np.float64).reshape(d, d)))
    return np.sum(terms, axis=-1) - const, (5 + 2 * levels(d) + levels(obs_t.size) + cond) * np.sum(forms, axis=-1) + 4 * np.abs(const)


def gauss_term(x, mean, cov, T=LD):
    """(-u^T u / 2 - sum_i log L_ii, size) of one point x (D,) under N(mean, cov), L = chol_lower(cov), L u = x - mean: the log-density without
    its constant D log(2 pi) / 2 (which cancels in the start term), as k_pf_start / k_pf_pin form it by forward substitution.  A careful fp64
    evaluation rounds, for row i with n_i = |x_i| + |mean_i| + sum_{j<i} |L_ij u_j|: the residual x_i - mean_i, the products L_ij u_j and the
    sum of these i + 1 terms as a tree ((2 + levels(i + 1)) n_i / L_ii in u_i), and the division (|u_i|).  That local error of u_i is carried
    into every later row by the substitution itself: e_i = local_i + sum_{j<i} |L_ij| e_j / L_ii.  The quadratic form then moves by
    sum_i |u_i| e_i, its squares and their tree add (1 + levels(D)) q / 2 with q = sum u_i^2, the factor L, whoever forms it in fp64, carries
    cond_2(cov) 2^-53 relative into q (cond_2(cov) q / 2), the logarithms are rounded once and added as a tree ((1 + levels(D)) sum |log L_ii|),
    each sees its L_ii off by a relative 2^-53 (D in all), and the last subtraction is rounded at no more than q / 2 + |sum log L_ii|."""
    x, mean = np.asarray(x, dtype=T).ravel(), np.asarray(mean, dtype=T).ravel()
    d = x.size
    cov64 = np.asarray(cov, dtype=np.float64).reshape(d, d)
    low = np.linalg.cholesky(cov64) if T is np.float64 else cholesky(np.asarray(cov64, dtype=T))
    low = np.asarray(low, dtype=T)
    u, err = np.zeros(d, dtype=T), np.zeros(d, dtype=T)
    for i in range(d):
        prods = low[i, :i] * u[:i]
        u[i] = ((x[i] - mean[i]) - _sum(prods, 0)) / low[i, i]
        n_i = np.abs(x[i]) + np.abs(mean[i]) + np.sum(np.abs(prods))
        err[i] = ((2 + levels(i + 1)) * n_i + np.sum(np.abs(low[i, :i]) * err[:i])) / low[i, i] + np.abs(u[i])
    q, logs = _sum(u * u, 0), np.log(np.diag(low))
    ld = _sum(logs, 0)
    size = (np.sum(np.abs(u) * err) + (1 + levels(d) + T(np.linalg.cond(cov64))) * q / 2 + (1 + levels(d)) * np.sum(np.abs(logs)) + d
            + (q / 2 + np.abs(ld)))
    return -q / 2 - ld, size


def start_term(x, mu0, tau0, m0, s0, T=LD):
    """(log N(x; mu0, tau0) - log N(x; m0, S0), size) of one start x (D,): the initial term of a drawn start under a prior, two gauss_term
    and their difference, rounded at no more than the sum of the two terms' magnitudes"""
    prior, size_p = gauss_term(x, mu0, tau0, T)
    law, size_l = gauss_term(x, m0, s0, T)
    return prior - law, size_p + size_l + np.abs(prior) + np.abs(law)


def statistics_rows(model, theta, dt, stored, T=LD):
    """The rows (Q, G, H) of stored stride-1 paths or lineages (n, Np, D): (rows (n, 3, D), sizes (n, 3, D)).  Q_j = sum_k r_j^2 / dt,
    G_j = sum_k phi_j r_j, H_j = sum_k dt phi_j^2 with r = x_k - x_{k-1} - dt f(x_{k-1}) (= dt d + eta), phi at x_{k-1}.  sizes: the
    recovery of r from the stored states, sum_k 2 |r_j| (|x_k,j| + |x_{k-1},j| + dt |f_j|) / dt for Q and the same with |phi_j| in
    2 |r_j| / dt's place for G, plus (1 + levels(Np - 1)) sum_k |summand| -- every summand once and the additions of the sum as a tree;
    H has that term alone."""
    x, dt = np.asarray(stored, dtype=T), T(dt)
    prev, new = x[:, :-1], x[:, 1:]
    f, _ = model_drift(model, theta, prev, T)
    phi = model_phi(model, prev, T)
    r = (new - prev) - dt * f
    reach = np.abs(new) + np.abs(prev) + dt * np.abs(f)
    sq, sg, sh = r * r / dt, phi * r, dt * (phi * phi)
    rows = np.stack((_sum(sq, 1), _sum(sg, 1), _sum(sh, 1)), axis=1)
    lv = levels(r.shape[1])      # (the Np - 1 summands of a row added as a tree; the recovery terms of Q and G dwarf it, H has nothing else)
    sizes = np.stack((_sum(2 * np.abs(r) * reach / dt + (1 + lv) * np.abs(sq), 1), _sum(np.abs(phi) * reach + (1 + lv) * np.abs(sg), 1),
                      (1 + lv) * _sum(np.abs(sh), 1)), axis=1)
    return rows, sizes


def normalised_weights(log_w, T=LD, total_scale=None):
    """W_i = w_i / sum w, w_i = exp(lw_i - max lw), and the size of each one's rounding in units of itself, 1 + |lw_i - max lw| (the
    argument of exp carries one rounding of a number of that size).  total_scale: the sum times it (a mutant's)."""
    lw = np.asarray(log_w, dtype=T)
    off = lw - np.max(lw, axis=-1, keepdims=True)
    w = np.exp(off)
    s = np.expand_dims(_sum(w, -1), -1)
    return w / (s if total_scale is None else s * T(total_scale)), 1 + np.abs(off)


def weighted_sum(log_w, values, T=LD, total_scale=None):
    """(sum_i W_i v_i, size) over the first axis of values (n, ...): size = sum_i W_i (1 + |lw_i - max lw|) |v_i| + 2 levels(n) sum_i W_i |v_i|
    -- the weights' own rounding, and the additions of two sums of n terms added as trees: the normalising sum, whose relative error every
    term inherits, and the sum itself"""
    w, size = normalised_weights(log_w, T, total_scale)
    v = np.asarray(values, dtype=T)
    w, size = w.reshape((-1,) + (1,) * (v.ndim - 1)), size.reshape((-1,) + (1,) * (v.ndim - 1))
    return _sum(w * v, 0), _sum(w * (size + 2 * levels(v.shape[0])) * np.abs(v), 0)


def stretch_weights(log_w, slots, T=LD):
    """The back-propagated weights of every stretch from the slot table of particle_paths(slots=arange(n)) -- slots (M + 1, n), row j the
    slot of final slot m's lineage in stretch j: W^j_a = sum_{m: slots[j][m] = a} W_m, (M + 1, n)"""
    w, _ = normalised_weights(log_w, T)
    slots = np.asarray(slots, dtype=np.int64)
    out = np.zeros(slots.shape, dtype=T)
    for j in range(slots.shape[0]):
        np.add.at(out[j], slots[j], w)
    return out


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
