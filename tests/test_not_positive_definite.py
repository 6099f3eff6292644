"""
GPU suite (-m gpu): the "S_t is not positive definite" contract of the Lorenz-96 energy kernels -- LinAlgError naming the problem, as
the reference raises from chol_inv (variational.py:380) -- beyond a first pivot that is negative everywhere:

  * operator level (Context.energy): the FIRST failing pivot j chosen by extended_ref.break_at_pivot -- first / last pivot of a 4-column
    panel, the last row, rows next to the padding, the later 64-blocks above D = 64 --, at one grid point t* only (above D = 64 one in
    each stream's half), with both want_hyper forms at D <= 64, and in one problem of a batch; the same call with that grid point
    repaired must then equal the oracle (no stale status word, no stale e_t);
  * fused path: one bad problem (first, last, and next to the 64-problem boundary), one bad grid point (0, through a per-problem s0
    with one negative eigenvalue; or N-1, through a rank-one spike in x), on the contexts of test_theta_gradient.SURVIVAL plus one
    problem at D = 12 and the time-chunked sweep at D = 72 (bad point in its second chunk); free_energy, sweep, gradient(x) and
    sweep_enqueue + fetch_f must all raise;
  * after the error: theta_gradient() and gradient(None) raise as well (never numbers), and the same context evaluated next on healthy
    inputs gives F and the gradient bit for bit equal to a fresh context's.

Every input is verified on the CPU by test_l96_energy_conditioning_cpu.py (the oracle raises exactly there and nowhere else, by a
margin that is no rounding).  The bad inputs only produce NaN arithmetic behind the kernels' early return; no address depends on them.
"""
import numpy as np
import pytest

import vgpa_amd as va
import vgpa_amd._lib as lib
import extended_ref as xr
from conftest import rel_err
from test_l96_energy_conditioning_cpu import (BATCHED_PIVOT, DT, FUSED, N_PTS, PIVOTS, THETA, bad_problems, bad_s0, fused_datasets,
                                              operator_inputs, oracle_energy, spike_last)

pytestmark = pytest.mark.gpu

TOL = 1e-9
NOT_PD = np.linalg.LinAlgError
_INPUTS, _FRESH = {}, {}


def _operator_reference(d, nb):
    if (d, nb) not in _INPUTS:
        inp = operator_inputs(d, (1e2,) * nb)
        _INPUTS[d, nb] = (inp, [oracle_energy(inp, k) for k in range(nb)])
    return _INPUTS[d, nb]


def _energy(ctx, inp, st, hyper):
    sl = (slice(None),) if st.shape[0] > 1 else (0,)
    return ctx.energy(inp["a"][sl], inp["b"][sl], inp["m"][sl], st[sl], want_edf=False, want_hyper=hyper)


def _assert_equals_oracle(out, orc, nb, hyper):
    names = ("Esde", "Ef", "Edf", "dEsde_dm", "dEsde_dS") + (("dEsde_dth", "dEsde_dsig") if hyper else ())
    for k in range(nb):
        for q, v in zip(names, out):
            if v is not None:
                assert rel_err(np.asarray(v)[k] if nb > 1 else v, orc[k][q]) <= TOL, (k, q)


OPERATOR = [(d, j, hyper) for d, js in PIVOTS.items() for j in js for hyper in ((False, True) if d <= 64 else (False,))]


@pytest.mark.parametrize("d,j,hyper", OPERATOR, ids=lambda v: str(v))
def test_first_failing_pivot_at_one_grid_point(d, j, hyper):
    inp, orc = _operator_reference(d, 1)
    ctx = va.Context("L96", "rk4", d, N_PTS, DT, sigma=inp["sigma"], theta=[THETA])
    for t in ((0, 2, N_PTS - 1) if d <= 64 else (0, N_PTS - 1)):       # (above D = 64: one grid point in each stream's half)
        st = inp["st"].copy()
        st[0, t] = xr.break_at_pivot(st[0, t], j)
        with pytest.raises(NOT_PD, match=r"problem 0:"):
            _energy(ctx, inp, st, hyper)
        _assert_equals_oracle(_energy(ctx, inp, inp["st"], hyper), orc, 1, hyper)      # that grid point repaired
    ctx.close()


@pytest.mark.parametrize("d,k,hyper", [(d, k, h) for d, k in BATCHED_PIVOT for h in ((False, True) if d <= 64 else (False,))])
def test_one_bad_problem_of_a_batch_at_operator_level(d, k, hyper):
    nb = 3
    inp, orc = _operator_reference(d, nb)
    ctx = va.Context("L96", "rk4", d, N_PTS, DT, sigma=inp["sigma"], theta=[THETA], batch=nb)
    st = inp["st"].copy()
    st[k, 2] = xr.break_at_pivot(st[k, 2], d - 1)
    with pytest.raises(NOT_PD, match=rf"problem {k}:"):
        _energy(ctx, inp, st, hyper)
    _assert_equals_oracle(_energy(ctx, inp, inp["st"], hyper), orc, nb, hyper)
    ctx.close()


# --------------------------------------------------------------------------------------------------------------------------------
def _fused_context(case, probs, s0_rows):
    """The case's context on the problems' own data and the given s0 per problem (e0 = 0: KL(q0 || p0) has no value at a bad s0).  The
    time-chunked sweep has no per-problem s0: one problem, the shared one."""
    _, d, nb, flag, chunk = case
    p0 = probs[0]
    ctx = va.Context("L96", p0.method, d, p0.n_pts, p0.dt, sigma=p0.sigma, theta=[float(p0.theta)], m0=p0.m0,
                     s0=s0_rows[0] if chunk else p0.s0, obs_t=p0.obs_t, obs_y=p0.obs_y, obs_noise=np.reshape(p0.obs_noise, (d, d)),
                     e0=0.0, batch=nb, flags=getattr(lib, flag) if flag else 0)
    if chunk:
        assert ctx.streaming and nb == 1 and chunk < p0.n_pts - 1
        ctx.set_option(lib.OPT_LD_CHUNK, chunk)
    else:
        _set_data(ctx, probs, s0_rows)
    return ctx


def _set_data(ctx, probs, s0_rows):
    """(every array again: None would put the shared value of vgpa_create back, not keep the rows of an earlier call)"""
    m, d = probs[0].obs_t.size, probs[0].dim_d
    ctx.set_problem_data(obs_y=np.stack([np.reshape(q.obs_y, (m, d)) for q in probs]), m0=np.stack([q.m0 for q in probs]),
                         s0=np.stack(s0_rows))


def _fresh(case):
    """F and the gradient of the healthy inputs on a context of their own: once per case"""
    if case[0] not in _FRESH:
        _, probs, xs = fused_datasets(case)
        ctx = _fused_context(case, probs, [q.s0 for q in probs])
        f, g = ctx.sweep(xs)
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
        _FRESH[case[0]] = (np.atleast_1d(f).copy(), np.asarray(g).copy())
        ctx.close()
    return _FRESH[case[0]]


FUSED_CASES = [pytest.param(case, k, where, id=f"{case[0]}-k{k}-{where}")
               for case in FUSED for k in bad_problems(case[2]) for where in ("first", "last")]


@pytest.mark.parametrize("case,k,where", FUSED_CASES)
def test_one_bad_problem_one_bad_grid_point_on_the_fused_path(case, k, where):
    """theta_gradient() behind the failed evaluation: the integrand kernels (k_energy_l96_r<NB, true>, lde_theta_integrand) flag a bad
    pivot themselves, but no path leads to a resident bad S_t except through a sweep that has flagged it already, so what is asserted
    is the outcome -- LinAlgError naming the problem --, not which of the two set the word."""
    _, probs, xs = fused_datasets(case)
    nb, chunk = case[2], case[4]
    good_s0 = [np.asarray(q.s0, dtype=float) for q in probs]
    s0_rows, x_bad = list(good_s0), np.array(xs)
    if where == "first":
        s0_rows[k] = bad_s0(probs[k], k)
    else:
        x_bad[k] = spike_last(probs[k], xs[k], k)
    f_want, g_want = _fresh(case)
    ctx = _fused_context(case, probs, s0_rows)
    match = rf"problem {k}:"
    for call in (ctx.free_energy, ctx.sweep, ctx.gradient):
        with pytest.raises(NOT_PD, match=match):
            call(x_bad)
    xb, gb = ctx.alloc(x_bad.size), ctx.alloc(x_bad.size)
    xb.upload(x_bad)
    ctx.sweep_enqueue(xb, gb)
    with pytest.raises(NOT_PD, match=match):
        ctx.fetch_f()
    ctx.release_x()
    xb.free(); gb.free()
    # after the error: never numbers
    with pytest.raises(NOT_PD, match=match):
        ctx.free_energy(x_bad)
    if chunk:
        with pytest.raises(RuntimeError):                          # (NotImplementedError: the time-chunked sweep has no dF/dtheta)
            ctx.theta_gradient()
    else:
        with pytest.raises(NOT_PD, match=match):
            ctx.theta_gradient()
    with pytest.raises((NOT_PD, RuntimeError)):
        ctx.gradient(None)
    # ... and a clean context on healthy inputs (the shared s0 of the time-chunked context cannot be replaced: a bad x only)
    if where == "first" and chunk:
        ctx.close()
        return
    if where == "first":
        _set_data(ctx, probs, good_s0)
    f, g = ctx.sweep(xs)
    ctx.close()
    assert np.array_equal(np.atleast_1d(f), f_want) and np.array_equal(np.asarray(g), g_want)
