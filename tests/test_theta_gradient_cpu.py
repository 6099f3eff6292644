"""
dF/dtheta at fixed (A_t, b_t) and the exact M-step in theta: the interface and the arithmetic, without a device.

The reference value everywhere is the central difference of the oracle's F in theta with step 0.5 per component: at fixed (A_t, b_t)
F is quadratic in theta (the drift is affine in theta, E_sde takes the diagonal of Sigma^-1, and m_t, S_t, E0, E_obs do not depend on
theta), so the difference quotient is exact up to rounding (<= 3e-13 relative on the fixtures).  Tolerance: the suite's 1e-9.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd.batch import theta_mstep
from conftest import load_golden
from oracle import vgpa_oracle as vo

TOL = 1e-9


def _f(p, x):
    return vo.free_energy(p, x, faithful=False)[0]


def _dth(p, x):
    return np.atleast_1d(np.asarray(vo.free_energy(p, x, faithful=False)[1]["dEsde_dth"], dtype=float))


def _shift(p, delta):
    th = np.asarray(p.theta, dtype=float) + delta
    return dataclasses.replace(p, theta=float(th) if th.ndim == 0 else th)


def fd_theta_gradient(p, x, step=0.5):
    """central difference of the oracle's F, one theta component at a time"""
    th = np.atleast_1d(np.asarray(p.theta, dtype=float))
    out = np.zeros(th.size)
    for i in range(th.size):
        e = np.zeros(th.size)
        e[i] = step
        d = e if th.size > 1 else float(e[0])
        out[i] = (_f(_shift(p, d), x) - _f(_shift(p, -d), x)) / (2.0 * step)
    return out


def l96_theta_gradient_numpy(p, x):
    """The value the Lorenz-96 kernels must compute: sum_i (Sigma^-1)_ii int UT-mean(f_i(chi) + (A chi)_i - b_i) dt, with the sigma
    points, the weights and the flat roll (quirk Q1) of the energy itself -- the residuals of E_sde summed BEFORE squaring."""
    lin_a, off_b = p.split(x)
    mt, st = vo.solve_fwd(p.method, p.dt, False, lin_a, off_b, p.m0, p.s0, p.sigma)
    isg = np.diag(p.inverse_sigma)
    d = p.dim_d
    kappa = 1.05 * d
    c = d + kappa
    w0, w = kappa / c, 1.0 / (2.0 * c)
    it = np.zeros(p.n_pts)
    for t in range(p.n_pts):
        low = np.linalg.cholesky(c * st[t])
        chi = np.concatenate((mt[t][np.newaxis, :], mt[t] + low.T, mt[t] - low.T))
        resid = vo.l96_drift(chi, p.theta) + chi.dot(lin_a[t].T) - off_b[t]
        it[t] = isg.dot(w0 * resid[0] + w * np.sum(resid[1:], axis=0))
    return p.dt * (np.sum(it) - 0.5 * (it[0] + it[-1]))


def test_symbol_and_methods_exist():
    assert "vgpa_theta_gradient" in va._lib.SYMBOLS
    assert hasattr(va.Context, "theta_gradient")
    for cls in (va.VarGP, va.ProblemBatch):
        assert hasattr(cls, "theta_gradient") and hasattr(cls, "fit_theta")


def test_header_declares_the_entry_point_and_keeps_the_abi():
    import os
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vgpa_hip.h")).read()
    assert "int vgpa_theta_gradient(vgpa_ctx* ctx, double* out);" in text
    assert va._lib.ABI_VERSION == 2


@pytest.mark.parametrize("tag", ["ou_rk4_p", "dw_rk4_p", "l63_rk4_p"])
def test_mstep_minimises_the_oracle_free_energy(tag):
    z = load_golden(tag)
    p = vo.Problem.from_fixture(z)
    x = z["x"]
    theta = np.atleast_1d(np.asarray(p.theta, dtype=float))
    g0, g1 = _dth(p, x), _dth(_shift(p, 1.0), x)
    # the reference's member IS dF/dtheta for these models
    assert np.max(np.abs(g0 - fd_theta_gradient(p, x))) <= TOL * np.max(np.abs(g0))
    new = theta_mstep(theta[None], g0[None], g1[None])[0]
    q = dataclasses.replace(p, theta=float(new[0]) if new.size == 1 else new)
    assert _f(q, x) <= _f(p, x)
    h = g1 - g0
    assert np.all(h > 0.0)
    assert np.all(np.abs(_dth(q, x)) <= TOL * (np.abs(g0) + np.abs(h * theta)))


def test_pooled_mstep_is_the_minimiser_of_the_summed_quadratic():
    zs = [load_golden(t) for t in ("ou_rk4_p", "ou_heun_p")]
    ps = [vo.Problem.from_fixture(z) for z in zs]
    xs = [z["x"] for z in zs]
    assert ps[0].theta == ps[1].theta
    theta = float(ps[0].theta)
    g0 = np.stack([_dth(p, x) for p, x in zip(ps, xs)])
    g1 = np.stack([_dth(_shift(p, 1.0), x) for p, x in zip(ps, xs)])
    new = theta_mstep(np.full((2, 1), theta), g0, g1, pooled=True)
    assert new.shape == (2, 1) and new[0, 0] == new[1, 0]
    # the parabola through the summed F at theta - 0.5, theta, theta + 0.5
    fm, fc, fp = (sum(_f(_shift(p, d), x) for p, x in zip(ps, xs)) for d in (-0.5, 0.0, 0.5))
    slope, curv = (fp - fm) / 1.0, (fp - 2.0 * fc + fm) / 0.25
    # (the second difference carries the rounding of F, ~1e-16 |F| / 0.25, against a curvature of order |F| / 10: ~1e-14 relative
    #  in the step, far inside the bound)
    assert abs(new[0, 0] - (theta - slope / curv)) <= 1e-8 * abs(theta)
    # own steps differ from the pooled one
    own = theta_mstep(np.full((2, 1), theta), g0, g1)
    assert own[0, 0] != own[1, 0]


@pytest.mark.parametrize("tag", ["l96d12_rk4_p", "l96d17_rk4_p"])
def test_l96_formula_is_the_derivative_of_the_computed_free_energy(tag):
    z = load_golden(tag)
    p = vo.Problem.from_fixture(z)
    want = fd_theta_gradient(p, z["x"])[0]
    got = l96_theta_gradient_numpy(p, z["x"])
    assert abs(got - want) <= TOL * abs(want), (got, want)
    # ... which the reference's member (from the closed-form mean drift) is not
    ref = float(np.sum(_dth(p, z["x"])))
    assert abs(ref - want) > 1e-3 * abs(want)
