"""
tests/extended_ref.py -- TEST INFRASTRUCTURE: the sweep of oracle/vgpa_oracle.py (forward and backward steppers, observation terms,
the four models' energies, the gradient assembly) in np.longdouble (x87 80-bit, 64-bit mantissa), and the seeded covariance generators
of the conditioning / not-positive-definite tests.

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
