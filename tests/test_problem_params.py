"""
Per-problem drift parameters and system noise (vgpa_set_problem_params / ProblemBatch(own_parameters=True)) on the GPU.

Problem k of a batch carries its own theta (theta_k = theta (1 + 0.05 (k mod 5))) and its own Sigma -- isotropic sigma_k^2 I with
its own sigma_k, diagonal non-isotropic, or dense SPD -- beside its own dataset (vgpa_set_problem_data).  Every problem is checked
against the numpy oracle evaluated with its own parameters (TOL = 1e-9 relative), on every kernel family the context picks.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_MATERIALIZE
from conftest import rel_err
from helpers import SEED, build_problem
from oracle import vgpa_oracle as vo
from test_problem_batch import FAMILIES, _context, _datasets

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _own_sigma(p, k, kind):
    """problem k's Sigma: sigma_k^2 I (iso; 1-D: sigma_k^2), a diagonal of distinct entries (diag), or dense SPD (dense)"""
    if p.single_dim:
        return float(p.sigma) * (1.0 + 0.1 * (k % 4))
    d = p.dim_d
    s = float(np.mean(np.diag(p.sigma)))
    if kind == "iso":
        return s * (1.0 + 0.1 * (k % 4)) * np.eye(d)
    if kind == "diag":
        return np.diag(s * (1.0 + 0.1 * ((np.arange(d) + k) % 3)))
    rho = 0.1 * (1 + k % 3)                         # (1 - rho) I + rho 11^T: SPD, no zero off the diagonal
    return s * (1.0 + 0.05 * (k % 4)) * ((1.0 - rho) * np.eye(d) + rho * np.ones((d, d)))


def _with_params(probs, kind):
    out = []
    for k, p in enumerate(probs):
        th = np.asarray(p.theta, dtype=float) * (1.0 + 0.05 * (k % 5))
        out.append(dataclasses.replace(p, theta=float(th) if th.ndim == 0 else th, sigma=_own_sigma(p, k, kind)))
    return out


def _set_params(ctx, probs):
    d = probs[0].dim_d
    ctx.set_problem_params(theta=np.stack([np.atleast_1d(q.theta) for q in probs]),
                           sigma=np.stack([np.reshape(q.sigma, (d, d)) for q in probs]))


def _check(ctx, probs, xs, checked, efx=True):
    f, g = ctx.sweep(xs)
    f, g = np.atleast_1d(f), np.reshape(g, (len(probs), -1))
    mt, st = np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st"))
    ef = np.asarray(ctx.fetch("Efx")) if efx else None
    for k in checked:
        f_o, g_o, state = vo.sweep(probs[k], xs[k], faithful=False)
        assert abs(f[k] - f_o) <= TOL * abs(f_o), (k, f[k], f_o)
        assert rel_err(g[k], g_o) <= TOL, k
        assert rel_err(mt[k].ravel(), np.ravel(state["mt"])) <= TOL, k
        assert rel_err(st[k].ravel(), np.ravel(state["st"])) <= TOL, k
        if efx:
            assert rel_err(ef[k].ravel(), np.ravel(state["Efx"])) <= TOL, k
    return f, g


def _checked(nb):
    return range(nb) if nb <= 8 else sorted(set(range(0, nb, 7)) | {1, 2, 3, nb - 1})


def _kinds(name, d):
    if name in ("OU", "DW"):
        return ("iso",)
    return ("iso", "diag", "dense") if name == "L63" or d == 12 else ("iso", "diag")


CASES = [(name, meth, d, tf, nb, fl, kind) for (name, meth, d, tf, sizes, alt) in FAMILIES for nb in sizes for fl in (0, alt)
         for kind in _kinds(name, d)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[2] or ''}-{c[1]}-B{c[4]}-f{c[5]}-{c[6]}")
def test_every_family_against_the_oracle(case):
    name, method, d, tf, nb, flags, kind = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    probs = _with_params(probs, kind)
    ctx = _context(base, probs, nb, flags, obs_t=False)       # own data (shared times) and, below, own parameters
    _set_params(ctx, probs)
    _check(ctx, probs, xs, _checked(nb))
    ctx.close()


@pytest.mark.parametrize("case", [("L63", "rk4", None, 1.0, 8), ("L63", "rk4", None, 1.0, 520), ("L96", "rk4", 12, 0.5, 4),
                                  ("OU", "heun", None, 2.0, 600)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_own_times_and_own_parameters_together(case):
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, True)
    probs = _with_params(probs, "diag")
    ctx = _context(base, probs, nb, 0, obs_t=True)
    _set_params(ctx, probs)
    _check(ctx, probs, xs, _checked(nb))
    ctx.close()


def _shared_context(p0, nb, flags=0):
    dd = p0.dim_d
    sig = np.array([[p0.sigma]]) if p0.single_dim else p0.sigma
    return va.Context(p0.model, p0.method, dd, p0.n_pts, p0.dt, sigma=sig, theta=np.atleast_1d(p0.theta), m0=np.atleast_1d(p0.m0),
                      s0=np.reshape(p0.s0, (dd, dd)), obs_t=p0.obs_t, obs_y=p0.obs_y, obs_noise=np.reshape(p0.obs_noise, (dd, dd)),
                      e0=float(np.asarray(vo.kl0(p0))), batch=nb, flags=flags)


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80), ("L63", "rk4", None, 1.0, 520)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_rows_equal_to_the_shared_parameters_are_bit_identical(case):
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False, nset=1)
    p0 = probs[0]
    ref = _shared_context(p0, nb)
    f0, g0 = ref.sweep(xs)
    ref.close()
    ctx = _shared_context(p0, nb)
    _set_params(ctx, [p0] * nb)
    f1, g1 = ctx.sweep(xs)
    ctx.close()
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80, "iso"), ("L96", "rk4", 17, 0.5, 8, "diag"),
                                  ("L63", "rk4", None, 1.0, 520, "dense"), ("OU", "euler", None, 2.0, 600, "iso")],
                         ids=lambda c: f"{c[0]}-B{c[4]}-{c[5]}")
def test_permuting_the_rows_permutes_the_results(case):
    name, method, d, tf, nb, kind = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    probs = _with_params(probs, kind)
    ctx = _context(base, probs, nb, 0, obs_t=False)
    _set_params(ctx, probs)
    f, g = ctx.sweep(xs)
    ctx.close()
    perm = np.random.default_rng(3).permutation(nb)
    ctx = _context(base, [probs[i] for i in perm], nb, 0, obs_t=False)
    _set_params(ctx, [probs[i] for i in perm])
    fp, gp = ctx.sweep(xs[perm])
    ctx.close()
    assert np.array_equal(fp, f[perm]) and np.array_equal(gp, g[perm])


def test_psit_and_lamt_of_the_fused_gradient_case():
    """L96 D = 40, RK4, 80 isotropic rows of their own sigma_k: the fragment-cover steppers with the fused backward + gradient kernel
    (from 64 problems on); Psi_t comes back through the Q'' recovery with each problem's own diag Sigma^-1."""
    base, probs, xs = _datasets("L96", "rk4", 0.5, 40, 80, False)
    probs = _with_params(probs, "iso")
    ctx = _context(base, probs, 80, 0, obs_t=False)
    _set_params(ctx, probs)
    ctx.sweep(xs)
    lam, psi = np.asarray(ctx.fetch("lamt")), np.asarray(ctx.fetch("psit"))
    for k in (0, 1, 2, 3, 41, 79):
        _, _, state = vo.sweep(probs[k], xs[k], faithful=False)
        assert rel_err(lam[k].ravel(), np.ravel(state["lamt"])) <= TOL, k
        assert rel_err(psi[k].ravel(), np.ravel(state["psit"])) <= TOL, k
    ctx.close()


@pytest.mark.parametrize("name,method,tf,d,kind", [("OU", "euler", 2.0, None, "iso"), ("L63", "rk4", 1.0, None, "dense"),
                                                   ("L96", "rk4", 0.5, 12, "diag")])
def test_hyper_parameter_members_per_problem(name, method, tf, d, kind):
    nb = 4
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    probs = _with_params(probs, kind)
    p0 = probs[0]
    dd, n = p0.dim_d, p0.n_pts
    states = [vo.sweep(q, x, faithful=False)[2] for q, x in zip(probs, xs)]
    a = xs[:, :n * dd * dd].reshape(nb, n, dd, dd)
    b = xs[:, n * dd * dd:].reshape(nb, n, dd)
    mt = np.stack([np.reshape(s["mt"], (n, dd)) for s in states])
    st = np.stack([np.reshape(s["st"], (n, dd, dd)) for s in states])
    ctx = _context(base, probs, nb, 0, obs_t=False)
    _set_params(ctx, probs)
    out = ctx.energy(a, b, mt, st, want_edf=False, want_hyper=True)
    ctx.close()
    dth, dsg = np.atleast_1d(out[5]), np.asarray(out[6])
    for k in range(nb):
        one = _shared_context(probs[k], 1)
        ek = one.energy(a[k:k + 1], b[k:k + 1], mt[k:k + 1], st[k:k + 1], want_edf=False, want_hyper=True)
        one.close()
        assert abs(np.atleast_1d(out[0])[k] - ek[0]) <= 1e-12 * abs(ek[0]), k
        assert rel_err(np.ravel(dth[k]), np.ravel(ek[5])) <= 1e-12, k
        assert rel_err(np.ravel(dsg[k]), np.ravel(ek[6])) <= 1e-12, k


@pytest.mark.parametrize("name,method,tf,d", [("OU", "euler", 2.0, None), ("L96", "rk4", 1.0, 12)])
def test_parameter_grid_optimisation_matches_single_problem_runs(name, method, tf, d):
    """one dataset at four theta points (and two sigma^2): every member ends where its own VarGP, optimised alone, ends"""
    ps = [build_problem(name, method, tf, dim_d=d, seed=SEED) for _ in range(4)]
    for k, p in enumerate(ps):
        th = np.asarray(p["model"].theta, dtype=float) * (1.0 + 0.1 * k)
        p["model"].theta = float(th) if th.ndim == 0 else th
        if k % 2:
            p["model"].sigma = 1.2 * (p["model"].sigma if np.ndim(p["model"].sigma) == 0 else np.asarray(p["model"].sigma))
    pb = va.ProblemBatch([p["vgp"] for p in ps], own_parameters=True)
    opts = {"max_it": 40}
    x, f, stats = pb.optimise(pb.initialization(), opts)
    assert len({round(float(v), 6) for v in f}) == 4
    for k, p in enumerate(ps):
        xk, fk = p["vgp"].device_scg(opts)(p["vgp"].initialization())
        assert abs(f[k] - fk) <= 1e-8 * abs(fk), (k, f[k], fk)
    ps[2]["model"].theta = ps[3]["model"].theta           # a member's theta changed: the context is rebuilt with it
    f2 = pb.free_energy(x)
    single = ps[2]["vgp"].free_energy(x[2])
    assert abs(f2[2] - single) <= 1e-12 * abs(single)
    pb.close()


def test_above_d64_own_theta_and_shared_sigma_only():
    base, probs, xs = _datasets("L96", "rk4", 0.5, 72, 3, False, nset=3)
    probs = [dataclasses.replace(p, theta=float(p.theta) * (1.0 + 0.05 * k)) for k, p in enumerate(probs)]
    ctx = _context(base, probs, 3, 0, obs_t=False)
    ctx.set_problem_params(theta=np.array([[float(q.theta)] for q in probs]))
    _check(ctx, probs, xs, [0, 1, 2], efx=False)
    sig = np.stack([np.asarray(q.sigma, dtype=float) * (1.0 + 0.1 * k) for k, q in enumerate(probs)])
    with pytest.raises(NotImplementedError):
        ctx.set_problem_params(sigma=sig)
    ctx.close()


def test_errors_keep_the_previous_parameters():
    base, probs, xs = _datasets("L96", "rk4", 0.5, 12, 4, False)
    probs = _with_params(probs, "diag")
    ctx = _context(base, probs, 4, 0, obs_t=False)
    _set_params(ctx, probs)
    f0, g0 = ctx.sweep(xs)
    with pytest.raises(ValueError):
        ctx.set_problem_params(theta=np.zeros((3, 1)))
    with pytest.raises(ValueError):
        ctx.set_problem_params(sigma=np.zeros((4, 12, 11)))
    bad = np.stack([np.asarray(q.sigma) for q in probs])
    bad[2] = -np.eye(12)
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        ctx.set_problem_params(sigma=bad)
    dense = bad.copy()
    dense[2] = np.ones((12, 12))                            # not positive definite, not diagonal
    with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
        ctx.set_problem_params(sigma=dense)
    f1, g1 = ctx.sweep(xs)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    ctx.close()
    base, probs, xs = _datasets("OU", "euler", 2.0, None, 4, False)
    probs = _with_params(probs, "iso")
    ctx = _context(base, probs, 4, 0, obs_t=False)
    _set_params(ctx, probs)
    f0, _ = ctx.sweep(xs)
    with pytest.raises(ValueError, match="problem 1"):
        ctx.set_problem_params(sigma=np.array([[[1.0]], [[0.0]], [[1.0]], [[1.0]]]))
    f1, _ = ctx.sweep(xs)
    assert np.array_equal(f0, f1)
    ctx.close()
