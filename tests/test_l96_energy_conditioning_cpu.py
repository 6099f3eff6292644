"""
The extended-precision reference of the Lorenz-96 energy (tests/extended_ref.py) and every input the GPU tests of the energy kernels
on ill-conditioned / not-positive-definite covariances use, checked without a device: the GPU modules
(test_l96_energy_conditioning.py, test_not_positive_definite.py) import their cases and constructions from here, so no GPU case rests
on an input that the reference itself might accept or reject by rounding.
"""
import dataclasses

import numpy as np
import pytest

import extended_ref as xr
from conftest import rel_err
from oracle import vgpa_oracle as vo

CONDS = (1e2, 1e4, 1e6, 1e8)
SMALL_D = (5, 8, 13, 17, 31, 40, 44, 45, 57, 64)       # padded / unpadded last panels, odd / even NB, partial / full update units
LARGE_D = (72, 130, 192, 330)                          # 130: a 2-row last diagonal block; 330: six blocks (> wpan = 4)
N_PTS, DT, THETA = 5, 0.01, 8.0
# first failing pivot j per D (operator level): first / last pivot of a panel, last row, padding-adjacent rows, later 64-blocks
PIVOTS = {13: (0, 3, 4, 12), 40: (0, 39), 64: (63,), 130: (0, 63, 64, 129), 330: (256, 329)}
BATCHED_PIVOT = ((40, 1), (130, 2))                    # (D, the one bad problem of a batch of three): last pivot, grid point 2
THETA_D = (13, 40, 72)                                 # theta-gradient cases (fused evaluation, S_t stays ill-conditioned)


def oracle_problem(d, sigma, n_pts=N_PTS, dt=DT, method="rk4", m0=None, s0=None):
    return vo.Problem(model="L96", method=method, dt=dt, theta=THETA, sigma=sigma, m0=m0, s0=s0, mu0=None, tau0=None,
                      obs_t=np.array([], dtype=np.int64), obs_y=None, obs_noise=None, n_pts=n_pts, dim_d=d)


def operator_inputs(d, conds, seed=0, n_pts=N_PTS):
    """The common inputs of the operator-level cases, one problem per entry of `conds`: m = 8 + randn, A = 8 I + 0.5 randn (dense,
    non-symmetric), b = randn, a diagonal Sigma with distinct entries (shared), S_t = spd_with_spectrum with its own Q per grid
    point.  Arrays carry the leading batch axis."""
    rng = np.random.default_rng([d, seed, 96])
    sigma = np.diag(3.0 + rng.random(d))
    nb = len(conds)
    m = 8.0 + rng.standard_normal((nb, n_pts, d))
    a = 8.0 * np.eye(d) + 0.5 * rng.standard_normal((nb, n_pts, d, d))
    b = rng.standard_normal((nb, n_pts, d))
    st = np.stack([np.stack([xr.spd_with_spectrum(rng, d, c) for _ in range(n_pts)]) for c in conds])
    return dict(d=d, sigma=sigma, a=a, b=b, m=m, st=st)


def oracle_energy(inp, k=0):
    """The fp64 oracle (lean) on problem k of operator_inputs, under the names of extended_ref.energy_l96."""
    p = oracle_problem(inp["d"], inp["sigma"], n_pts=inp["m"].shape[1])
    esde, (ef, edf), (dm, ds, dth, dsg) = vo.model_energy(p, inp["a"][k], inp["b"][k], inp["m"][k], inp["st"][k], faithful=False)
    return dict(Esde=esde, Ef=ef, Edf=edf, dEsde_dm=dm, dEsde_dS=ds, dEsde_dth=dth, dEsde_dsig=dsg)


def extended_energy(inp, k=0):
    return xr.energy_l96(THETA, inp["sigma"], DT, inp["a"][k], inp["b"][k], inp["m"][k], inp["st"][k])


def theta_inputs(d, nb, seed=0, n_pts=6, dt=1e-3, method="rk4"):
    """A fused evaluation whose S_t stays ill-conditioned: s0 = spd_with_spectrum(cond 1e4) per problem, dt = 1e-3, Sigma = 1e-4 diag.
    Returns the oracle problems (own m0, s0 each) and their x."""
    rng = np.random.default_rng([d, nb, seed, 7])
    sigma = 1e-4 * np.diag(3.0 + rng.random(d))
    probs, xs = [], []
    for _ in range(nb):
        p = oracle_problem(d, sigma, n_pts=n_pts, dt=dt, method=method, m0=8.0 + rng.standard_normal(d),
                           s0=xr.spd_with_spectrum(rng, d, 1e4))
        obs_t = np.array([2], dtype=np.int64)
        p = dataclasses.replace(p, obs_t=obs_t, obs_y=8.0 + rng.standard_normal((1, d)), obs_noise=np.eye(d), mu0=np.ones(d),
                                tau0=0.5 * np.eye(d))
        a = 8.0 * np.eye(d) + 0.5 * rng.standard_normal((n_pts, d, d))
        b = 8.0 * p.m0 + rng.standard_normal((n_pts, d))
        probs.append(p)
        xs.append(np.concatenate((a.ravel(), b.ravel())))
    return probs, np.stack(xs)


# --------------------------------------------------------------------------- #
#  Fused-path constructions of the not-positive-definite tests: one bad problem, one bad grid point
# --------------------------------------------------------------------------- #
# (id, D, B, flag name or None, chunk of the time-chunked sweep or None): the Lorenz-96 contexts of test_theta_gradient.SURVIVAL, one
# problem at D = 12, and the time-chunked sweep at D = 72 (one problem, shared s0; chunk < n_pts)
FUSED = [("d40-B3", 40, 3, None, None), ("d40-B65", 40, 65, None, None), ("d17-B4-generic", 17, 4, "FLAG_FORCE_GENERIC", None),
         ("d72-B2", 72, 2, None, None), ("d12-B1", 12, 1, None, None), ("d72-streamed", 72, 1, "FLAG_STREAM_LARGE_D", 30)]
FUSED_TF, FUSED_METHOD = 0.5, "rk4"
_FUSED = {}


def bad_problems(nb):
    return sorted({0, nb - 1} | ({63, 64} if nb == 65 else set()))


def fused_datasets(case):
    """test_problem_batch._datasets of the case, once."""
    if case[0] not in _FUSED:
        from test_problem_batch import _datasets
        _, d, nb, _, _ = case
        _FUSED[case[0]] = _datasets("L96", FUSED_METHOD, FUSED_TF, d, nb, False)
    return _FUSED[case[0]]


def bad_s0(q, seed=0):
    """q.s0 with the eigenvalue along one random direction u replaced by -1e-4: not positive definite at grid point 0 only (one step
    later dt Sigma_uu has lifted it far above zero again; checked below)."""
    rng = np.random.default_rng([seed, 13])
    u = rng.standard_normal(q.dim_d)
    u /= np.linalg.norm(u)
    s0 = np.asarray(q.s0, dtype=float)
    s0 = s0 - (u.dot(s0).dot(u) + 1e-4) * np.outer(u, u)
    return (s0 + s0.T) / 2.0


def bad_set(q, x, s0=None):
    """The grid points where the oracle's forward sweep is not positive definite (smallest eigenvalue < -1e-6 lambda_max), after
    asserting that every other one is safely positive definite (>= 1e-3 lambda_max)."""
    a, b = q.split(x)
    _, st = vo.solve_fwd(q.method, q.dt, False, a, b, q.m0, q.s0 if s0 is None else s0, q.sigma)
    bad = set()
    for t in range(q.n_pts):
        lam = np.linalg.eigvalsh(st[t])
        if lam[0] < -1e-6 * lam[-1]:
            bad.add(t)
        else:
            assert lam[0] >= 1e-3 * lam[-1], (t, lam[0], lam[-1])
    return bad


def spike_last(q, x, seed=0):
    """x with a rank-one spike (beta / dt) u u^T in the A_t that only the LAST step of the stepper reads -- A_{N-2} for Euler, A_{N-1}
    for Heun / RK2 / RK4 (their last step reads A_{N-2} too, but so does the step before it) -- sized by a search over beta with the
    oracle: the first beta that leaves S_{N-1}, and no other grid point, not positive definite.  Along u the last step multiplies
    S by the stepper's stability polynomial in beta, which is negative in a window only (RK4: 1 - b + b^2/2 - b^3/6 < 0 from 1.6 on)."""
    rng = np.random.default_rng([seed, 17])
    d, n = q.dim_d, q.n_pts
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    t = n - 2 if q.method == "euler" else n - 1
    for beta in (1.25, 1.5, 1.75, 2.0, 2.5, 3.0, 4.0):
        y = np.array(x, dtype=float)
        y[:n * d * d].reshape(n, d, d)[t] += (beta / q.dt) * np.outer(u, u)
        try:
            if bad_set(q, y) == {n - 1}:
                return y
        except AssertionError:
            pass
    raise AssertionError(f"no spike makes S_(N-1) alone indefinite under {q.method}")


# --------------------------------------------------------------------------- #
#  Tests
# --------------------------------------------------------------------------- #
def test_longdouble_is_the_80_bit_format():
    """A host without 80-bit arithmetic must fail HERE, not quietly degrade the GPU tests to an fp64 yardstick."""
    assert np.finfo(np.longdouble).eps <= 1.1e-19


@pytest.mark.parametrize("d", [13, 40, 130])
def test_factor_and_inverse_at_cond_1e8(d):
    """L L^T = S relative to max|S|; L^-1 L = I relative to max(|L^-1| |L|), the scale of the products that are summed."""
    s = xr.spd_with_spectrum(np.random.default_rng(d), d, 1e8)
    assert np.array_equal(s, s.T)
    lam = np.linalg.eigvalsh(s)
    assert abs(lam[-1] / lam[0] / 1e8 - 1.0) < 1e-6
    low = xr.cholesky(s)
    inv = xr.tri_inverse(low)
    e_f = float(np.max(np.abs(low.dot(low.T) - s)) / np.max(np.abs(s)))
    e_i = float(np.max(np.abs(inv.dot(low) - np.eye(d))) / np.max(np.abs(inv).dot(np.abs(low))))
    print(d, e_f, e_i)
    assert e_f <= 1e-17 and e_i <= 1e-17
    assert np.array_equal(np.triu(low, 1), np.zeros((d, d))) and np.array_equal(np.triu(inv, 1), np.zeros((d, d)))


@pytest.mark.parametrize("cond", [1.0, 1e2])
@pytest.mark.parametrize("d", [5, 13, 40, 72])
def test_equals_the_fp64_oracle_when_well_conditioned(d, cond):
    inp = operator_inputs(d, (cond,), seed=3)
    want, got = oracle_energy(inp), extended_energy(inp)
    for key, val in want.items():
        err = rel_err(got[key], val)
        print(d, cond, key, err)
        assert err <= 1e-12, key


def test_trapezoid_between_observations_and_forward_sweep():
    rng = np.random.default_rng(2)
    fx = rng.standard_normal((23, 3))
    for obs in (None, [], [0, 7, 22], [4, 9]):
        want = vo.my_trapz(fx, 0.01, obs if obs else None)
        assert rel_err(xr.my_trapz(fx, 0.01, obs), want) <= 1e-14
    (p,), x = theta_inputs(13, 1)
    a, b = p.split(x[0])
    for method in ("euler", "heun", "rk2", "rk4"):
        m_o, s_o = vo.solve_fwd(method, p.dt, False, a, b, p.m0, p.s0, p.sigma)
        m_x, s_x = xr.solve_fwd(method, p.dt, a, b, p.m0, p.s0, p.sigma)
        assert rel_err(m_x, m_o) <= 1e-14 and rel_err(s_x, s_o) <= 1e-14, method


@pytest.mark.parametrize("d,j", [(d, j) for d, js in PIVOTS.items() for j in js])
def test_break_at_pivot_fails_at_that_pivot_and_nowhere_else(d, j):
    inp = operator_inputs(d, (1e2,))
    oracle_energy(inp)                                                 # S as generated: no error
    s = inp["st"][0, 2]
    broken = xr.break_at_pivot(s, j)
    assert np.array_equal(broken, broken.T) and np.count_nonzero(broken != s) == 1
    with pytest.raises(np.linalg.LinAlgError, match=f"pivot {j}"):     # ... the first pivot to fail is j, in extended precision
        xr.cholesky(broken)
    low = xr.cholesky(s)
    col = broken[j:, j] - low[j:, :j].dot(low[j, :j])
    assert abs(float(col[0] / low[j, j] ** 2) + 1e-3) < 1e-9           # by the margin asked for
    for t in (0, 2, N_PTS - 1):
        bad = dict(inp, st=inp["st"].copy())
        bad["st"][0, t] = xr.break_at_pivot(inp["st"][0, t], j)
        with pytest.raises(np.linalg.LinAlgError):
            oracle_energy(bad)
        with pytest.raises(np.linalg.LinAlgError):
            extended_energy(bad)


@pytest.mark.parametrize("d,k", BATCHED_PIVOT)
def test_batched_break_is_in_one_problem_only(d, k):
    inp = operator_inputs(d, (1e2,) * 3)
    bad = dict(inp, st=inp["st"].copy())
    bad["st"][k, 2] = xr.break_at_pivot(inp["st"][k, 2], d - 1)
    for i in range(3):
        if i == k:
            with pytest.raises(np.linalg.LinAlgError):
                oracle_energy(bad, i)
        else:
            oracle_energy(bad, i)
        oracle_energy(inp, i)


@pytest.mark.parametrize("d", THETA_D)
def test_theta_gradient_inputs_stay_ill_conditioned(d):
    probs, xs = theta_inputs(d, 3)
    for p, x in zip(probs, xs):
        a, b = p.split(x)
        _, st = vo.solve_fwd(p.method, p.dt, False, a, b, p.m0, p.s0, p.sigma)
        conds = [np.linalg.cond(s) for s in st]
        print(d, ["%.1e" % c for c in conds])
        assert min(conds) >= 1e3
        vo.free_energy(p, x, faithful=False)                           # ... and positive definite throughout


@pytest.mark.parametrize("case", FUSED, ids=lambda c: c[0])
def test_fused_constructions_are_bad_exactly_where_intended(case):
    _, probs, xs = fused_datasets(case)
    nb = case[2]
    for k in range(nb) if nb <= 4 else bad_problems(nb):
        assert bad_set(probs[k], xs[k]) == set()
    for k in bad_problems(nb):
        q = probs[k]
        assert bad_set(q, xs[k], s0=bad_s0(q, k)) == {0}
        assert bad_set(q, spike_last(q, xs[k], k)) == {q.n_pts - 1}
        with pytest.raises(np.linalg.LinAlgError):
            vo.model_energy(q, *q.split(xs[k]), *vo.solve_fwd(q.method, q.dt, False, *q.split(xs[k]), q.m0, bad_s0(q, k), q.sigma),
                            faithful=False)
        y = spike_last(q, xs[k], k)
        with pytest.raises(np.linalg.LinAlgError):
            vo.free_energy(q, y, faithful=False)
