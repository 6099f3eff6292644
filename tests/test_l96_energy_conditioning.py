"""
GPU suite (-m gpu): the Lorenz-96 energy kernels on ILL-CONDITIONED covariances, against the extended-precision reference of
tests/extended_ref.py.  Operator level (Context.energy), so S_t is exactly what the test chooses: spd_with_spectrum, condition
1e2 ... 1e8, a different rotation per grid point (the suite's other inputs have cond(S_t) <= 2.3, where the panel updates and the
substitution contribute at the 1e-5 level and a loss of accuracy there hides below the 1e-9 tolerance).

  * k_energy_l96_r<NB> (want_hyper=False) and k_energy_l96<NB> (want_hyper=True) at D = 5 ... 64: padded and unpadded last panels, odd
    and even NB, partial and full units of the panel update;
  * the blocked factorisation above D = 64 (large_d_energy.hip): D = 130 has a 2-row last diagonal block, D = 330 six blocks (two-level
    trailing update, a ragged level of the inverse by halves); five grid points are uneven halves on the two streams;
  * the batch axis, a different condition number per problem;
  * k_energy_l96_r<NB, true> / lde_theta_integrand (theta_gradient()) behind a fused evaluation whose S_t stays at cond >= 1e3.

Tolerance, per case and quantity q, in conftest.rel_err's norm:  err_k(q) <= max(FACTOR * err_o(q), 64 D 2^-53)  with err_o the fp64
oracle (LAPACK) against the extended reference and err_k the kernel against it.  FACTOR = 32 is five bits over LAPACK: the allowance for
an explicit blocked L^-1 and for MFMA accumulation chains that sum in another order; the floor covers the quantities the oracle has
exact to the last bit.  Every case prints both errors and their ratio.
"""
import numpy as np
import pytest

import vgpa_amd as va
import extended_ref as xr
from conftest import rel_err
from oracle import vgpa_oracle as vo
from test_l96_energy_conditioning_cpu import (CONDS, DT, LARGE_D, N_PTS, SMALL_D, THETA, THETA_D, extended_energy, operator_inputs,
                                              oracle_energy, theta_inputs)

pytestmark = pytest.mark.gpu

FACTOR = {1e2: 32, 1e4: 32, 1e6: 32, 1e8: 32}
QUANTITIES = ("Esde", "Ef", "Edf", "dEsde_dm", "dEsde_dS")
HYPER = ("dEsde_dth", "dEsde_dsig")
_REF = {}


def _reference(d, conds):
    """inputs, extended reference and fp64 oracle per problem: once per (D, conds), shared by the want_hyper forms"""
    key = (d, tuple(conds))
    if key not in _REF:
        inp = operator_inputs(d, conds)
        _REF[key] = (inp, [extended_energy(inp, k) for k in range(len(conds))], [oracle_energy(inp, k) for k in range(len(conds))])
    return _REF[key]


def _floor(d):
    return 64.0 * d * 2.0 ** -53


def _assert_close(tag, d, cond, got, ext, orc, names):
    worst = 0.0
    fails = []
    for q in names:
        err_o, err_k = rel_err(orc[q], ext[q]), rel_err(got[q], ext[q])
        bound = max(FACTOR[cond] * err_o, _floor(d))
        ratio = err_k / err_o if err_o > 0.0 else float("inf") if err_k > 0.0 else 0.0
        print(f"{tag} cond={cond:.0e} {q}: err_o={err_o:.2e} err_k={err_k:.2e} ratio={ratio:.2f} bound={bound:.2e}")
        if err_k > _floor(d):
            worst = max(worst, ratio)
        if not err_k <= bound:
            fails.append((q, err_o, err_k, bound))
    print(f"{tag} cond={cond:.0e} WORST ratio above the floor: {worst:.2f}")
    assert not fails, fails


def _run(d, conds, hyper):
    inp, ext, orc = _reference(d, conds)
    nb = len(conds)
    ctx = va.Context("L96", "rk4", d, N_PTS, DT, sigma=inp["sigma"], theta=[THETA], batch=nb)
    sl = (slice(None),) if nb > 1 else (0,)
    out = ctx.energy(inp["a"][sl], inp["b"][sl], inp["m"][sl], inp["st"][sl], want_hyper=hyper)
    ctx.close()
    names = QUANTITIES + (HYPER if hyper else ())
    for k, cond in enumerate(conds):
        got = {q: (np.asarray(v)[k] if nb > 1 else v) for q, v in zip(names, out)}
        family = "lde" if d > 64 else "l96" if hyper else "l96_r"
        _assert_close(f"[{family}] D={d} B={nb} k={k}", d, cond, got, ext[k], orc[k], names)


@pytest.mark.parametrize("hyper", [False, True], ids=["l96_r", "l96"])
@pytest.mark.parametrize("cond", CONDS, ids=lambda c: f"{c:.0e}")
@pytest.mark.parametrize("d", SMALL_D)
def test_one_wave_kernels(d, cond, hyper):
    _run(d, (cond,), hyper)


@pytest.mark.parametrize("cond", CONDS, ids=lambda c: f"{c:.0e}")
@pytest.mark.parametrize("d", LARGE_D)
def test_blocked_factorisation_above_d64(d, cond):
    _run(d, (cond,), False)


@pytest.mark.parametrize("hyper", [False, True], ids=["plain", "hyper"])
@pytest.mark.parametrize("d", [40, 130])
def test_batch_axis_with_a_condition_number_per_problem(d, hyper):
    _run(d, (1e2, 1e4, 1e6), hyper)


def _theta_context(probs, nb):
    p0 = probs[0]
    d = p0.dim_d
    ctx = va.Context("L96", p0.method, d, p0.n_pts, p0.dt, sigma=p0.sigma, theta=[THETA], m0=p0.m0, s0=p0.s0, obs_t=p0.obs_t,
                     obs_y=p0.obs_y, obs_noise=p0.obs_noise, e0=0.0, batch=nb)
    if nb > 1:
        ctx.set_problem_data(obs_y=np.stack([q.obs_y for q in probs]), m0=np.stack([q.m0 for q in probs]),
                             s0=np.stack([q.s0 for q in probs]))
    return ctx


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("d", THETA_D)
def test_theta_gradient_on_ill_conditioned_states(d, nb):
    """theta_gradient() against the central difference, step 0.5, of the extended-precision E_sde over the extended-precision forward
    sweep (E_sde is quadratic in theta); err_o is the same difference quotient of the fp64 oracle.  cond(S_t) >= 1e3 at every grid point
    (asserted by test_theta_gradient_inputs_stay_ill_conditioned): the bound is the one of cond 1e4."""
    probs, xs = theta_inputs(d, nb)
    ctx = _theta_context(probs, nb)
    ctx.free_energy(xs if nb > 1 else xs[0])
    g = np.asarray(ctx.theta_gradient()).reshape(nb)
    ctx.close()
    fails = []
    for k, (p, x) in enumerate(zip(probs, xs)):
        a, b = p.split(x)
        mt, st = xr.solve_fwd(p.method, p.dt, a, b, p.m0, p.s0, p.sigma)
        want = xr.theta_gradient_fd(THETA, p.sigma, p.dt, a, b, mt, st)
        m64, s64 = vo.solve_fwd(p.method, p.dt, False, a, b, p.m0, p.s0, p.sigma)
        e_up, e_dn = (vo.energy_l96(THETA + s, p.inverse_sigma, p.dt, a, b, m64, s64, [], faithful=False)[0] for s in (0.5, -0.5))
        err_o, err_k = rel_err(e_up - e_dn, want), rel_err(g[k], want)
        bound = max(FACTOR[1e4] * err_o, 64.0 * d * 2.0 ** -53)
        print(f"[theta] D={d} B={nb} k={k}: dF/dtheta={g[k]:.15e} err_o={err_o:.2e} err_k={err_k:.2e} bound={bound:.2e}")
        if not err_k <= bound:
            fails.append((k, err_o, err_k, bound))
    assert not fails, fails
