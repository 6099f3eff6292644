"""
dF/dtheta from the resident sweep state (vgpa_theta_gradient) and the estimation of theta (fit_theta) on the GPU.

Reference value: the central difference of the oracle's F in theta with step 0.5 per component -- exact for the quadratic F is in
theta at fixed (A_t, b_t); its rounding noise on the fixtures is <= 3e-13 relative.  Tolerance: the suite's TOL = 1e-9 (max-norm
relative, conftest.rel_err).  For OU / DW / L63 the reference's own dEsde_dth (golden data) is compared as well.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_MATERIALIZE, FLAG_STREAM_LARGE_D, FLAG_SYM_UNITS
from conftest import rel_err
from helpers import SEED, build_problem, problem_from_golden
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import gpu_context, make_problem
from test_problem_batch import _context, _datasets
from test_problem_params import _set_params, _with_params
from test_theta_gradient_cpu import fd_theta_gradient

pytestmark = pytest.mark.gpu

TOL = 1e-9
_FD = {}


def _reference(tag, prob, x):
    """the difference quotient of the oracle, once per fixture"""
    if tag not in _FD:
        _FD[tag] = fd_theta_gradient(prob, x)
    return _FD[tag]


@pytest.mark.parametrize("flags", [0, FLAG_FORCE_GENERIC, FLAG_SYM_UNITS], ids=["fast", "generic", "sym"])
def test_golden_fixtures(golden, flags):
    p = problem_from_golden(golden, flags)
    if flags == FLAG_SYM_UNITS and not (str(golden["model"]) == "L96" and 5 <= p["d"] <= 44):
        return                                     # (the flag selects a kernel family there only: nothing else to run)
    v = p["vgp"]
    v.free_energy(golden["x"])
    g = np.atleast_1d(v.theta_gradient())
    want = _reference(golden["_tag"], vo.Problem.from_fixture(golden), golden["x"])
    print(golden["_tag"], flags, g, want)
    assert g.shape == want.shape
    assert rel_err(g, want) <= TOL
    if str(golden["model"]) != "L96":              # the reference's member is dF/dtheta for these models
        assert rel_err(g, np.atleast_1d(golden["dEsde_dth"])) <= TOL
    # theta_gradient(x) evaluates F at x first: the same value
    assert np.array_equal(np.atleast_1d(v.theta_gradient(golden["x"])), g)
    # shape of model.theta
    assert np.shape(v.theta_gradient()) == np.shape(p["model"].theta)


@pytest.mark.parametrize("flags", [0, FLAG_FORCE_GENERIC], ids=["fast", "generic"])
@pytest.mark.parametrize("name,method,tf,d", [("OU", "Heun", 2.0, None), ("DW", "RK2", 2.0, None), ("L63", "RK4", 1.5, None),
                                               ("L96", "RK4", 1.0, 16), ("L96", "RK4", 1.0, 40)])
def test_fresh_seeded_inputs(name, method, tf, d, flags):
    """Inputs that are NOT in the fixtures: seed 7, dense non-symmetric A (as test_against_oracle_on_fresh_seeded_inputs)."""
    p = build_problem(name, method, tf, 0.01, d, seed=7, flags=flags)
    v = p["vgp"]
    x = v.initialization() + 0.05 * np.random.default_rng(3).standard_normal(v.dim_n * v.dim_d * (v.dim_d + 1))
    z = dict(model=name, method=method, dt=0.01, theta=p["model"].theta, sigma=p["model"].sigma, m0=p["m0"],
             s0=p["s0"], mu0=p["mu0"], tau0=p["tau0"], obs_t=p["obs_t"], obs_y=p["obs_y"], obs_noise=p["obs_noise"],
             time_window=p["model"].time_window)
    prob = vo.Problem.from_fixture({k: np.asarray(val) for k, val in z.items()})
    g = np.atleast_1d(v.theta_gradient(x))
    want = _reference((name, method, d), prob, x)
    print(name, method, d, flags, g, want)
    assert rel_err(g, want) <= TOL


# (model, method, D, tf, B, flags): the lane path (B = 600), the four-kernel path (MATERIALIZE), 16 lanes per problem (L63, B = 5), the
# L96 energy kernel behind role-specialised / cover steppers (B = 3) and behind the backward kernel that assembles the gradient (B = 65)
BATCHED = [("L96", "rk4", 40, 0.5, 3, 0), ("L96", "rk4", 40, 0.5, 65, 0), ("OU", "heun", None, 2.0, 600, 0),
           ("OU", "heun", None, 2.0, 600, FLAG_MATERIALIZE), ("L63", "rk4", None, 1.0, 600, 0),
           ("L63", "rk4", None, 1.0, 600, FLAG_MATERIALIZE), ("L63", "rk4", None, 1.0, 5, 0)]


@pytest.mark.parametrize("own_params", [False, True], ids=["data", "data+params"])
@pytest.mark.parametrize("case", BATCHED, ids=lambda c: f"{c[0]}{c[2] or ''}-B{c[4]}-f{c[5]}")
def test_batched_rows_equal_single_problem_contexts(case, own_params):
    name, method, d, tf, nb, flags = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    if own_params:
        probs = _with_params(probs, "iso")
    ctx = _context(base, probs, nb, flags, obs_t=False)
    if own_params:
        _set_params(ctx, probs)
    ctx.free_energy(xs)
    g = np.asarray(ctx.theta_gradient())
    ctx.close()
    assert g.shape == (nb, 3 if name == "L63" else 1)
    worst = 0.0
    for k, q in enumerate(probs):
        one = gpu_context(q, flags=flags)
        one.free_energy(xs[k])
        gk = np.asarray(one.theta_gradient())
        one.close()
        worst = max(worst, rel_err(g[k], gk))
    print(case, own_params, "worst row vs single-problem context", worst)
    assert worst <= TOL
    for k in sorted({0, 1, nb // 2, nb - 1}):
        want = fd_theta_gradient(probs[k], xs[k])
        assert rel_err(g[k], want) <= TOL, (k, g[k], want)


@pytest.mark.parametrize("d,n", [(72, 9), (96, 8)])
def test_above_d64(d, n):
    p, x = make_problem("L96", d, n)
    ctx = gpu_context(p)
    ctx.free_energy(x)
    g = np.asarray(ctx.theta_gradient())
    ctx.close()
    want = fd_theta_gradient(p, x)
    print(d, g, want)
    assert g.shape == (1,) and rel_err(g, want) <= TOL
    # a batch with per-problem theta (Sigma is shared above D = 64)
    nb = 3
    probs = [dataclasses.replace(p, theta=float(p.theta) * (1.0 + 0.05 * k)) for k in range(nb)]
    xs = np.stack([x + 0.01 * np.random.default_rng(k).standard_normal(x.size) for k in range(nb)])
    ctx = gpu_context(p, batch=nb)
    ctx.free_energy(xs)
    g_shared = np.asarray(ctx.theta_gradient())
    ctx.set_problem_params(theta=np.array([[float(q.theta)] for q in probs]))
    ctx.free_energy(xs)
    g_own = np.asarray(ctx.theta_gradient())
    ctx.close()
    for k in range(nb):
        assert rel_err(g_shared[k], fd_theta_gradient(p, xs[k])) <= TOL, k
        assert rel_err(g_own[k], fd_theta_gradient(probs[k], xs[k])) <= TOL, k


SURVIVAL = [("L96", "rk4", 40, 0.5, 3, 0), ("L96", "rk4", 40, 0.5, 65, 0), ("L96", "rk4", 17, 0.5, 4, FLAG_FORCE_GENERIC),
            ("L96", "rk4", 72, 0.5, 2, 0), ("OU", "heun", None, 2.0, 600, 0), ("OU", "heun", None, 2.0, 600, FLAG_MATERIALIZE),
            ("L63", "rk4", None, 1.0, 600, 0), ("L63", "rk4", None, 1.0, 600, FLAG_MATERIALIZE), ("L63", "rk4", None, 1.0, 5, 0)]


@pytest.mark.parametrize("case", SURVIVAL, ids=lambda c: f"{c[0]}{c[2] or ''}-B{c[4]}-f{c[5]}")
def test_cached_state_survives(case):
    """gradient(None), fetch("psit") and energy_parts() behind theta_gradient() are bit for bit what they are without it -- F-only state
    of a context whose backward kernel assembles the gradient (B = 65), packed layouts, a lane context without materialised arrays."""
    name, method, d, tf, nb, flags = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False)

    def run(between):
        out = {}
        for what in ("gradient", "psit", "parts"):
            ctx = _context(base, probs, nb, flags, obs_t=False)
            ctx.free_energy(xs)
            if between:
                out["th"] = np.asarray(ctx.theta_gradient())
            if what == "gradient":
                out[what] = np.asarray(ctx.gradient(None))
                if between:                        # and once more behind the gradient: the same value
                    assert np.array_equal(np.asarray(ctx.theta_gradient()), out["th"])
            elif what == "psit":
                out[what] = np.asarray(ctx.fetch("psit"))
            else:
                out[what] = np.stack([np.atleast_1d(v) for v in ctx.energy_parts()])
            ctx.close()
        return out

    a, b = run(True), run(False)
    for what in ("gradient", "psit", "parts"):
        assert np.array_equal(a[what], b[what]), what


def test_errors():
    base, probs, xs = _datasets("L96", "rk4", 0.5, 12, 4, False)
    ctx = _context(base, probs, 4, 0, obs_t=False)
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.theta_gradient()
    ctx.free_energy(xs)
    ctx.theta_gradient()
    _set_params(ctx, _with_params(probs, "diag"))
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.theta_gradient()
    ctx.close()
    p, x = make_problem("L96", 72, 9)
    st = gpu_context(p, flags=FLAG_STREAM_LARGE_D)
    assert st.streaming
    st.free_energy(x)
    with pytest.raises(NotImplementedError):
        st.theta_gradient()
    st.close()
    ode = va.Context("NONE", "rk4", 3, 10, 0.01, sigma=np.eye(3))
    with pytest.raises(RuntimeError):
        ode.theta_gradient()
    ode.close()


@pytest.mark.parametrize("case", [("OU", "heun", None, 2.0, 8, False), ("L63", "rk4", None, 1.0, 4, True),
                                  ("L96", "rk4", 40, 0.5, 2, False)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_fit_theta(case):
    name, method, d, tf, nb, own = case
    ps = [build_problem(name, method, tf, dim_d=d, seed=SEED + k) for k in range(nb)]
    if own:
        for k, p in enumerate(ps):
            p["model"].theta = np.asarray(p["model"].theta, dtype=float) * (1.0 + 0.02 * k)
    pb = va.ProblemBatch([p["vgp"] for p in ps], own_parameters=own)
    rounds = 3
    theta0 = pb._theta_rows()
    x, f, theta, trace = pb.fit_theta(pb.initialization(), rounds, {"max_it": 15})
    assert trace["F"].shape == (rounds, 2, nb) and theta.shape == theta0.shape
    tot = trace["F"].sum(axis=2).ravel()
    print(case, "sum F per entry:", tot, "theta:", theta0[0], "->", theta[0])
    for a, b in zip(tot[:-1], tot[1:]):
        assert b <= a + 1e-9 * abs(a), tot
    for k, p in enumerate(ps):
        assert np.array_equal(np.atleast_1d(np.asarray(p["model"].theta, dtype=float)), theta[k])
    if not own:
        assert np.all(theta == theta[:1])
    # stationarity of the last M-step: dF/dtheta at the returned (x, theta) against the gradients that step was computed from
    g = pb.theta_gradient(x)
    pb.close()
    prev = trace["theta"][-2] if rounds > 1 else theta0
    g0, h = trace["g0"][-1], trace["g1"][-1] - trace["g0"][-1]
    if own:
        assert np.all(np.abs(g) <= 1e-9 * (np.abs(g0) + np.abs(h * prev))), (g, g0, h)
    else:
        gs, g0s, hs = g.sum(axis=0), g0.sum(axis=0), h.sum(axis=0)
        assert np.all(np.abs(gs) <= 1e-9 * (np.abs(g0s) + np.abs(hs * prev[0]))), (gs, g0s, hs)


def test_vargp_fit_theta_is_a_batch_of_one():
    p = build_problem("DW", "rk2", 2.0, seed=SEED)
    v = p["vgp"]
    x, f, theta, trace = v.fit_theta(v.initialization(), 2, {"max_it": 10})
    assert x.shape == (v.dim_n * 2,) and isinstance(f, float) and isinstance(theta, float)
    assert trace["F"].shape == (2, 2, 1) and p["model"].theta == theta
    assert abs(v.free_energy(x) - f) <= 1e-12 * abs(f)
    g0, h = trace["g0"][-1, 0, 0], trace["g1"][-1, 0, 0] - trace["g0"][-1, 0, 0]
    assert abs(v.theta_gradient()) <= 1e-9 * (abs(g0) + abs(h * trace["theta"][-2, 0, 0]))
