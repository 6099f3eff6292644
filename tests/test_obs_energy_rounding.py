"""
GPU suite (-m gpu): the observation terms, the closed-form energies of OU / double well / Lorenz-63, dF/dtheta and the fused paths of the
small models other than the lane pass held to ROUNDING ERROR -- against the longdouble restatement (tests/extended_ref.py), with the fp64
oracle's own error against it as the yardstick.  The inputs, the case tables and the references come from
test_obs_energy_rounding_cpu.py, which asserts their regimes without a device.

The bound is test_stepper_rounding's, unchanged: err_k(q) <= FACTOR * max(err_o(q), 2^-53), FACTOR = 32, in conftest.rel_err's norm
evaluated in longdouble.  For the scalar sums of terms of either sign (E_obs, every component of dEsde_dth and of dF/dtheta) the floor
is kappa 2^-53, kappa = sum |summand| / |sum summand| from the restatement (see the CPU module).  No other tolerance; bit equalities
(an explicit identity H against H = None, a per-problem parameter row against a single-problem context, rows off the observations
against zero) are bit equalities.

Every case asserts what ctx.plan() / ctx.resident() expose before a number, and prints err_o / err_k / ratio (/ kappa) for every
quantity.  Which observation kernel a case runs follows launch_obs (there is no counter for it): Context.obs_energy runs k_obs<false>
up to D = 64 and k_obs_nd + k_obs_fin above (the context then has the per-observation buffer; asserted through plan["fwd"] ==
"large_d"), k_obs<true> once vgpa_set_problem_obs_model gave the rows their own model, and k_obs_dense<PM> for the dense jump arrays;
a.diag is set for a diagonal R with H = None or an explicit identity.  A fused sweep runs k_obs_lane<D, PM> on the lane pass and
k_obs<PM> everywhere else (with the packed S_t where the plan has `packed`).

Measured on an MI355X (profiles/obs_energy_rounding_gputests.log has every compared problem; err_o is computed on the host of the same
run).  No kernel and no host constant of the parent commit exceeded its bound.  1308 comparisons; the kappa term decided none of them
(every one also met FACTOR * max(err_o, 2^-53)); worst kappa 46.9 (dEsde_dth of Lorenz-63, residual-cancels), 19.5 for dF/dtheta, 1.7
for E_obs.  Worst ratio err_k / max(err_o, kappa 2^-53) per kernel and quantity:
  k_energy_1d             E_sde 1.17, <f> 1.39, <df/dx> 1.00, dEsde_dm 2.01, dEsde_dS 3.84, dEsde_dth 1.82, dEsde_dSigma 1.02
  k_energy_l63            E_sde 2.15, <f> 1.50, <df/dx> 0.96, dEsde_dm 1.39, dEsde_dS 1.87, dEsde_dth 15.35, dEsde_dSigma 2.76
  k_obs<false>            1-D: E_obs 1.00, vector jump 1.10, matrix jump 0.21;  a.diag: 1.06, 1.00, 1.00;  dense: 3.15, 1.16, 1.17
                          (1-D includes the scalar operator h = 1.3)
  k_obs_nd + k_obs_fin    a.diag: E_obs 0.31, jumps 1.00;  wave per row: E_obs 23.95 (D = 72, M = 1, R of cond 1e4: err_o 1.5e-15, err_k
                          3.5e-14 -- the oracle whitens with the Cholesky factor, the kernel contracts with Q = H R^-1 H^T; both jumps of the
                          same case, which carry the same inverse, stand at err_o 5.5e-14 ... 7.7e-14), vector jump 1.73, matrix jump 0.96
  k_obs<true>, k_obs_dense<true>   1-D (shared h = 1.3): 1.00, 1.00, 0.38;  a.diag: 1.22, 1.00, 1.00;  dense: 3.21, 3.24, 3.25
  k_theta_lane            dF/dtheta 7.42
  hyp_only + k_trapz_multi   dF/dtheta 25.44 (Lorenz-63, generic steppers, Np = 2, residual-cancels: one component at err_o 3.6e-16, err_k
                          9.2e-15, its neighbours at err_o 6e-14)
  vgpa_fetch (k_edf_dense)   <f> 1.68, <df/dx> 1.00
  fused (check_fused of test_stepper_rounding, same log)   16 lanes per problem: F 2.92, Psi_t 2.65, E_obs 2.24, the rest below 2;
                          VGPA_FLAG_MATERIALIZE: E_sde 1.97, the rest below 2;  VGPA_FLAG_FORCE_GENERIC: E_sde 8.99, the rest below 2
  fused with a dense R / non-identity H (1-D: r = 0.07, h = 1.3)   k_obs<false> on the six paths above: E_sde 3.23, gLa 1.98, lam_t 1.83, gLb
                          1.80, dEsde_dm 1.43, the rest <= 1.00;  packed S_t (D = 36): E_sde 3.20, gLa 1.63, gLb 1.59, Psi_t 1.45 (recovery term
                          never needed), S_t 1.33;  k_obs_lane<1, false>: <= 1.00;  k_obs_lane<1, true>: gLa 1.13, the rest 1.00;  k_obs<true>:
                          E_sde 3.23, Psi_t 1.82, F, gradient, E_obs, lam_t 1.81;  k_obs_lane<3, true>: E_sde 3.23, F, gradient, E_obs 1.81
The module takes 16 s (12 s of them the first case: the device start and the imports).
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from test_gpu_edge_cases import fused_grad_switch, gpu_context, helper_switch
from test_kernel_paths import expected_plan
from test_obs_energy_rounding_cpu import (DT, ENERGY_CASES, FUSED_OBS_CASES, MODEL_D, OBS_CASES, OBS_PM_CASES, O_QUANTITIES,
                                          SMALL_FUSED_CASES, THETA_CASES, ObsCase, case_id, checked, compare, energy_inputs, energy_reference,
                                          fused_obs_kernel, fused_obs_problem, fused_obs_quantities, fused_obs_reference, obs_inputs, obs_kernel, obs_pm_inputs,
                                          obs_pm_reference, obs_reference, pm_count, small_fused_drift, takes_diag_branch, theta_inputs,
                                          theta_problem, theta_reference)
from test_stepper_rounding import FETCHED, MATRIX_KEYS, check_fused, psi_recovery_term, run_fused
from test_stepper_rounding import WORST as STEPPER_WORST
from test_stepper_rounding_cpu import FUSED_QUANTITIES

pytestmark = pytest.mark.gpu
WORST = {}                 # kernel -> quantity -> the worst ratio err_k / max(err_o, kappa 2^-53) of this process's run
PASSES = {}                # the comparisons of this process's run: how many, how many only the kappa term let pass, the worst kappa
TAKEN_OVER = dict(cached=False, moments="row_major", S="whole", dEs="whole", bwd="none", terms=False)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _flags(name):
    return getattr(_lib, name) if name else 0


def _plan_of(model, d, method, batch, flags, sigma, n_pts):
    return expected_plan(model, d, method, batch, flags, sigma, _n_cu(), n_pts=n_pts, fused_grad=fused_grad_switch(), helpers=helper_switch())


def _held(tag, kernel, got, ext, orc, kappas):
    return compare(tag, got, ext, orc, kappas, WORST.setdefault(kernel, {}), PASSES)


# ---- energies, operator level -----------------------------------------------------------------------------------------------

def _energy_context(c, theta, sigma, batch):
    d = MODEL_D[c.model]
    return va.Context(c.model, "euler", d, c.n_pts, DT, sigma=np.reshape(sigma, (d, d)), theta=np.atleast_1d(theta), batch=batch)


def _energy_call(ctx, c, inputs):
    """Context.energy on the stacked problems: a dict over the case's quantities, every value with the leading batch axis"""
    nb, d, n = len(inputs), MODEL_D[c.model], c.n_pts
    a, b, m, s = (np.stack([inp[i] for inp in inputs]) for i in (2, 3, 4, 5))
    out = ctx.energy(a, b, m, s, want_hyper=c.hyper)
    got = dict(Esde=np.reshape(out[0], (nb,)), Ef=np.reshape(out[1], (nb, n, d)), Edf=np.reshape(out[2], (nb, n, d, d)),
               dEsde_dm=np.reshape(out[3], (nb, n, d)), dEsde_dS=np.reshape(out[4], (nb, n, d, d)))
    if c.hyper:
        got["dEsde_dth"], got["dEsde_dsig"] = np.reshape(out[5], (nb, -1)), np.reshape(out[6], (nb, d, d))
    return got


@pytest.mark.parametrize("c", ENERGY_CASES, ids=case_id)
def test_closed_form_energies_operator_level(c):
    """k_energy_1d (OU, double well; Np across one block of 256) and k_energy_l63 (Np across one block of 64): E_sde, <f>, <df/dx>,
    dEsde_dm, dEsde_dS and, with want_hyper, dEsde_dth and dEsde_dSigma as the operator-level kernels write them -- benign, every-moment
    and residual-cancels inputs, one problem and three; the last case of a model has per-problem theta / sigma rows, each equal bit for
    bit to a single-problem context of its own."""
    inputs = [energy_inputs(c, k) for k in range(c.batch)]
    ctx = _energy_context(c, inputs[0][0], inputs[0][1], c.batch)
    assert ctx.plan()["fwd"] == _plan_of(c.model, MODEL_D[c.model], "euler", c.batch, 0, "diag", c.n_pts)["fwd"]
    if c.own:
        d = MODEL_D[c.model]
        ctx.set_problem_params(theta=np.stack([np.atleast_1d(inp[0]) for inp in inputs]),
                               sigma=np.stack([np.reshape(inp[1], (d, d)) for inp in inputs]))
    got = _energy_call(ctx, c, inputs)
    assert ctx.resident() == dict(TAKEN_OVER, terms=True), ctx.resident()      # (nothing cached; the energy kernel left its per-grid-point terms)
    ctx.close()
    kernel = "k_energy_l63" if c.model == "L63" else "k_energy_1d"
    fails = []
    for k in range(c.batch):
        ext, orc, kappas = energy_reference(c, k)
        fails += _held(f"[energy {case_id(c)}] k={k}", kernel, {q: got[q][k] for q in ext}, ext, orc, kappas if c.hyper else {})
        if c.own:
            one = _energy_context(c, inputs[k][0], inputs[k][1], 1)
            alone = _energy_call(one, c, inputs[k:k + 1])
            one.close()
            for q in ext:
                assert np.array_equal(alone[q][0], got[q][k]), (k, q)
    assert not fails, fails


# ---- observation terms, operator level --------------------------------------------------------------------------------------

def _obs_context(p, d, n_pts, obs_h):
    return va.Context("NONE", "euler", d, n_pts, DT, sigma=np.eye(d), obs_t=p.obs_t, obs_y=p.obs_y,
                      obs_noise=np.reshape(np.asarray(p.obs_noise, dtype=float), (d, d)), obs_h=obs_h)


@pytest.mark.parametrize("c", OBS_CASES, ids=case_id)
def test_observation_terms_operator_level(c):
    """Context.obs_energy: E_obs, the vector jump and the matrix jump of k_obs<false> (1-D: M = 1, 256, 257; n-D: M D across 256, both
    branches of a.diag), of k_obs_nd + k_obs_fin above D = 64 (D = 72, 257; the wave-per-row branch ragged at both) and of
    k_obs_dense<false> (jumps at index 0, at Np - 1 and at adjacent indices; every other row exactly zero).  An explicit identity H
    takes the diagonal path: bit for bit the result of H = None."""
    p, m, s = obs_inputs(c)
    ctx = _obs_context(p, c.d, c.n_pts, p.obs_h)
    assert (ctx.plan()["fwd"] == "large_d") == (obs_kernel(c) == "k_obs_nd") == (c.d > 64), ctx.plan()
    e, jm, js = ctx.obs_energy(m, s)
    assert ctx.resident() == TAKEN_OVER, ctx.resident()
    ctx.close()
    ext, orc, kappas, _ = obs_reference(c)
    got = dict(Eobs=e, jm=np.reshape(jm, np.shape(ext["jm"])), js=np.reshape(js, np.shape(ext["js"])))
    off = np.setdiff1d(np.arange(c.n_pts), p.obs_t)
    assert not np.any(got["jm"][off]) and not np.any(got["js"][off])
    if c.h_form == "eye":
        q, m2, s2 = obs_inputs(ObsCase(c.d, c.m_obs, c.n_pts, c.r_form, None, c.scale))
        plain = _obs_context(q, c.d, c.n_pts, None)
        e2, jm2, js2 = plain.obs_energy(m2, s2)
        plain.close()
        assert e2 == e and np.array_equal(jm2, jm) and np.array_equal(js2, js)
    kernel = obs_kernel(c) + (".diag" if takes_diag_branch(c) else ".dense") if c.d > 1 else "k_obs.1d"
    fails = _held(f"[obs {case_id(c)}]", kernel, {q: got[q] for q in O_QUANTITIES}, ext, orc, kappas)
    assert not fails, fails


@pytest.mark.parametrize("c", OBS_PM_CASES, ids=case_id)
def test_observation_terms_with_a_per_problem_model(c):
    """k_obs<true> and k_obs_dense<true>: ragged counts (1, the capacity, one between), a different R_k (and H_k) per problem, each
    problem's own observation times; 3 problems and 66.  The rows behind a problem's count hold NaN observations: nothing may read them."""
    d, nb, cap = MODEL_D[c.model], c.batch, c.capacity
    data = [obs_pm_inputs(c, k) for k in range(nb)]
    p0 = data[0][0]
    theta = [10.0, 28.0, 2.667] if c.model == "L63" else [1.0]
    rows_t = np.stack([v[3] for v in data])
    rows_y = np.stack([np.reshape(v[4], (cap, d)) for v in data]).astype(float)
    counts = np.array([pm_count(c, k) for k in range(nb)], dtype=np.int64)
    for k in range(nb):
        rows_y[k, counts[k]:] = np.nan
    ctx = va.Context(c.model, "rk4", d, c.n_pts, DT, sigma=np.eye(d), theta=theta, m0=np.ones(d), s0=0.2 * np.eye(d), obs_t=data[0][3],
                     obs_y=np.reshape(data[0][4], (cap, d)), obs_noise=np.reshape(np.asarray(p0.obs_noise, dtype=float), (d, d)), obs_h=p0.obs_h,
                     batch=nb)
    assert ctx.plan() == _plan_of(c.model, d, "rk4", nb, 0, "iso", c.n_pts), ctx.plan()
    ctx.set_problem_obs_model(n_obs=counts, obs_noise=np.stack([np.reshape(np.asarray(v[0].obs_noise, dtype=float), (d, d)) for v in data]),
                              obs_h=None if d == 1 or p0.obs_h is None else np.stack([v[0].obs_h for v in data]))
    ctx.set_problem_data(obs_t=rows_t, obs_y=rows_y)
    m = np.stack([np.reshape(v[1], (c.n_pts, d)) for v in data])
    s = np.stack([np.reshape(v[2], (c.n_pts, d, d)) for v in data])
    e, jm, js = ctx.obs_energy(m, s)
    assert ctx.resident() == TAKEN_OVER, ctx.resident()
    ctx.close()
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(jm)) and np.all(np.isfinite(js))
    fails = []
    for k in checked(nb):
        ext, orc, kappas, _ = obs_pm_reference(c, k)
        off = np.setdiff1d(np.arange(c.n_pts), data[k][0].obs_t)
        assert not np.any(jm[k][off]) and not np.any(js[k][off]), k
        got = dict(Eobs=e[k], jm=np.reshape(jm[k], np.shape(ext["jm"])), js=np.reshape(js[k], np.shape(ext["js"])))
        fails += _held(f"[obs-pm {case_id(c)}] k={k}", "k_obs<true>." + ("1d" if d == 1 else c.form), got, ext, orc, kappas)
    assert not fails, fails


# ---- dF/dtheta --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", THETA_CASES, ids=case_id)
def test_theta_gradient_behind_a_fused_evaluation(c):
    """vgpa_theta_gradient: k_theta_lane on the lane pass (Np = 2, 3, 4: the prefetch clamps; the chunk edges of 16 (1-D) and 4
    (Lorenz-63) grid points; 63 | 64 | 65 problems) and the hyp_only launches of k_energy_1d / k_energy_l63 + k_trapz_multi everywhere else
    (16 lanes per problem, FLAG_MATERIALIZE, FLAG_FORCE_GENERIC; Np = 2, 257, 258), with the host scaling by Sigma^-1 -- shared and
    per-problem theta, the three energy regimes and an integrand that changes sign."""
    d, nb, flags = MODEL_D[c.model], c.batch, _flags(c.flag)
    base, _ = theta_problem(c.model, c.n_pts, c.regime)
    ctx = gpu_context(base, batch=nb, flags=flags)
    plan = ctx.plan()
    assert plan == _plan_of(c.model, d, base.method, nb, flags, "diag", c.n_pts), plan
    assert plan["lane_pass"] == (c.path == "lane"), plan
    if c.path == "hyp":
        assert plan["fwd"] == ("generic" if c.flag == "FLAG_FORCE_GENERIC" else "wave" if nb == 5 else "lane"), plan
    if c.own:
        ctx.set_problem_params(theta=np.stack([np.atleast_1d(theta_inputs(c, k)[0].theta) for k in range(nb)]))
    xs = np.stack([theta_inputs(c, k)[1] for k in range(nb)])
    ctx.free_energy(xs if nb > 1 else xs[0])
    res = ctx.resident()
    assert res["cached"] and (res["moments"] == "time_major") == (c.path == "lane"), res
    g = np.reshape(ctx.theta_gradient(), (nb, -1))
    ctx.close()
    kernel = "k_theta_lane" if c.path == "lane" else "hyp_only+k_trapz_multi"
    fails = []
    for k in checked(nb):
        ext, orc, kappas = theta_reference(c, k)
        fails += _held(f"[theta {case_id(c)}] k={k}", kernel, dict(dFdth=g[k]), ext, orc, kappas)
    assert not fails, fails


# ---- fused sweeps of the small models other than the lane pass --------------------------------------------------------------

@pytest.mark.parametrize("c", SMALL_FUSED_CASES, ids=case_id)
def test_fused_paths_of_the_small_models(c):
    """Lorenz-63 on 16 lanes per problem (ode_wave.hip; k_energy_l63, k_obs, k_grad_small, k_reduce), the four-kernel path of
    VGPA_FLAG_MATERIALIZE for all three models and the generic steppers of VGPA_FLAG_FORCE_GENERIC: F, the gradient, E_sde, E_obs, m_t, S_t,
    lam_t, Psi_t, dEsde_dm, dEsde_dS -- benign and near the optimum -- and <f>, <df/dx> as vgpa_fetch serves them (k_edf_dense)."""
    p, plan, res, got = run_fused(c, FUSED_QUANTITIES, FETCHED + ("Efx", "Edf"))
    if c.family == "wave63":
        assert plan["fwd"] == plan["bwd"] == "wave", plan
    elif c.family == "materialize":
        assert not plan["lane_pass"] and plan["fwd"] == "lane", plan
    else:
        assert plan["fwd"] == plan["bwd"] == "generic", plan
    assert res["cached"] and (res["S"], res["dEs"], res["bwd"]) == ("whole", "whole", "psi"), res
    check_fused(c, p, plan, got, FUSED_QUANTITIES)
    # <f> and <df/dx> of the cached state (the fused sweep skips the dense <df/dx>: vgpa_fetch builds it)
    fails = []
    for k in checked(c.batch):
        ext, orc = small_fused_drift(c, k)
        fails += _held(f"[fused {case_id(c)}] k={k} drift", "fetch(Efx, Edf)", dict(Efx=got["Efx"][k], Edf=got["Edf"][k]), ext, orc, {})
    assert not fails, fails


@pytest.mark.parametrize("c", FUSED_OBS_CASES, ids=case_id)
def test_fused_sweeps_with_a_dense_or_per_problem_observation_model(c):
    """Three observations whose indices differ from their counters, R dense with cond 1e4 and H = I + 0.1 noise (or a diagonal R with
    distinct entries; the 1-D models: r = 0.07 and the scalar operator h = 1.3), behind a fused sweep: k_obs<false> on every path of
    test_fused_paths_of_the_small_models (Lorenz-63 on 16 lanes per problem; OU, double well and Lorenz-63 on the four-kernel path; double
    well and Lorenz-63 on the generic steppers) and reading the PACKED S_t of the isotropic cover kernels (D = 36); k_obs_lane<1, false>
    with h = 1.3; k_obs_lane<1, true> (3, 66, 130 problems), k_obs<true> (3, 66) and k_obs_lane<3, true> (520) with ragged counts and a
    model per problem.  Off the lane pass lam_t, Psi_t (which the jumps built from K and jsc enter directly), dEsde_dm and dEsde_dS are
    fetched and compared as well."""
    nb, d, flags = c.batch, c.d, _flags(c.flag)
    probs = [fused_obs_problem(c, k) for k in range(nb)]
    base, p0 = probs[0][2], probs[0][0]
    ctx = gpu_context(dataclasses.replace(base, obs_noise=p0.obs_noise, obs_h=p0.obs_h), batch=nb, flags=flags)
    plan = ctx.plan()
    assert plan == _plan_of(c.model, d, c.method, nb, flags, c.sigma, c.n_pts), plan
    assert plan["lane_pass"] == (c.family == "lane_pass") and plan["packed"] == (c.family == "packed"), plan
    assert (plan["fwd"] == "wave") == (c.family == "wave63") and (plan["fwd"] == "generic") == (c.family == "generic_small"), plan
    if c.pm:
        ctx.set_problem_obs_model(n_obs=np.array([v[0].obs_t.size for v in probs], dtype=np.int64),
                                  obs_noise=np.stack([np.reshape(np.asarray(v[0].obs_noise, dtype=float), (d, d)) for v in probs]),
                                  obs_h=None if d == 1 or p0.obs_h is None else np.stack([v[0].obs_h for v in probs]))
    xs = np.stack([v[1] for v in probs])
    f, g = ctx.sweep(xs if nb > 1 else xs[0])
    res = ctx.resident()
    assert res["cached"] and (res["S"] == "packed") == (c.family == "packed"), res
    f, g = np.atleast_1d(f), np.reshape(g, (nb, -1))
    names = fused_obs_quantities(c)
    fetched = {q: np.reshape(ctx.fetch(q), (nb, c.n_pts) + ((d, d) if q in MATRIX_KEYS else (d,))) for q in FETCHED if q in names}
    _, es, eo = ctx.energy_parts()
    es, eo = np.atleast_1d(es), np.atleast_1d(eo)
    ctx.close()
    k_a = c.n_pts * d * d
    fails = []
    for k in checked(nb):
        ext, orc, kappas = fused_obs_reference(c, k)
        got = dict(F=f[k], gLa=g[k][:k_a], gLb=g[k][k_a:], Esde=es[k], Eobs=eo[k], **{q: v[k] for q, v in fetched.items()})
        extra = {"psit": psi_recovery_term(probs[k][0], probs[k][1], ext["psit"])} if plan["store_q"] else None
        fails += compare(f"[fused-obs {case_id(c)}] k={k}", {q: got[q] for q in names}, ext, orc, kappas,
                         WORST.setdefault(fused_obs_kernel(c) + (".packed" if c.family == "packed" else ""), {}), PASSES, extra)
    assert not fails, fails


def test_worst_ratios_of_the_module():
    """The worst ratio err_k / max(err_o, kappa 2^-53) per kernel and quantity over the cases above that ran in this process (after them
    in file order), the number of comparisons, how many passed only through the kappa term, and the worst kappa: printed for the log."""
    for kernel, w in WORST.items():
        print(f"WORST [{kernel}]", " ".join(f"{q}={r:.2f}" for q, r in w.items()))
    for family in ("wave63", "materialize", "generic_small"):          # (check_fused keeps its ratios in test_stepper_rounding.WORST)
        print(f"WORST [{family}]", " ".join(f"{q}={r:.2f}" for (f, q), r in STEPPER_WORST.items() if f == family))
    print("PASSES", PASSES)
