"""
GPU suite (-m gpu): the forward stepper, the backward stepper and the gradient assembly of every kernel family held to ROUNDING ERROR
-- against the longdouble restatement of the sweep (tests/extended_ref.py), with the fp64 oracle's own error against it as the yardstick.
The inputs, the case tables and the references come from test_stepper_rounding_cpu.py, which asserts their regimes without a device.

The bound, per case, per compared problem and per quantity q, in conftest.rel_err's norm evaluated in longdouble (gLa and gLb each on
its own block; F, E_sde and E_obs as relative scalars):

    err_k(q) <= FACTOR * max(err_o(q), 2^-53)                                                  FACTOR = 32

err_o: the oracle against the restatement; err_k: the kernel against the restatement; 2^-53: the unit roundoff, for a quantity the oracle
happens to hit to the last bit; FACTOR: the allowance of test_l96_energy_conditioning.py -- five bits over the reference arithmetic, for
accumulation chains that sum in another order.  One derived extra term, for Psi_t alone and only where the plan has store_q: see
psi_recovery_term.  The older GPU tests keep TOL = 1e-9 against the oracle: they assert paths, layouts and bookkeeping on the benign inputs;
this module is where the arithmetic is held tight, on the benign inputs, on stiff dense A_t and near the optimum of the objective.

Every case asserts its plan (and, fused level, the record of the buffers) before a number, and prints err_o, err_k and their ratio
err_k / max(err_o, 2^-53) for every quantity.

Measured on an MI355X (profiles/stepper_rounding_gputests.log has every compared problem; err_o is computed on the host of the same run).  No kernel of the parent commit exceeded its bound; the recovery term was never what let a case pass
(worst Psi_t ratio where it applies: 1.93).  Worst ratio err_k / max(err_o, 2^-53) per family, with the quantity that gave it:
  operator level   lane 1.84 (Psi_t 9.6e-17 -> 2.0e-16), wave 1.77 (m_t 2.3e-16 -> 4.1e-16), role-specialised 1.53 (Psi_t 2.8e-16 -> 4.2e-16),
                   symmetric units 2.29 (S_t 4.5e-16 -> 1.0e-15), generic 1.69 (m_t 1.7e-16 -> 2.9e-16), D > 64 1.39 (m_t 1.6e-16 -> 2.3e-16)
  fused level      cover kernels 3.88 (E_sde 2.3e-17 -> 4.3e-16; gLb 2.45, gLa 2.34, lam_t 2.24, Psi_t 1.93), role-specialised 2.07 (dEsde_dS
                   2.6e-14 -> 5.5e-14), VGPA_FLAG_SYM_UNITS 2.69 (E_sde), symmetric units 1.68 (gLa 1.1e-14 -> 1.8e-14), VGPA_FLAG_KEEP_PSI
                   2.80 (E_sde), diagonal Sigma 1.80 (gLb 5.8e-14 -> 1.0e-13), generic 2.12 (gLa 2.5e-14 -> 5.4e-14), resident D = 72 2.74
                   (dEsde_dm 3.6e-15 -> 9.9e-15), time-chunked D = 72 1.78 (lam_t), lane pass 9.53 (E_sde 1.3e-16 -> 1.2e-15; F 5.13, gLa 3.16)
Worst err_o / err_k / ratio per quantity:
  operator level   m_t 3.6e-16 / 4.1e-16 / 1.77, S_t 1.0e-15 / 1.0e-15 / 2.29, lam_t 2.1e-16 / 2.1e-16 / 1.64, Psi_t 5.2e-16 / 1.1e-15 / 2.18
  fused, D >= 12   F 1.9e-16 / 2.1e-16 / 1.89, gLa 3.1e-14 / 5.4e-14 / 2.34, gLb 2.4e-13 / 3.8e-13 / 2.45, E_sde 6.8e-16 / 8.7e-16 / 3.88,
                   E_obs 3.4e-16 / 2.7e-16 / 2.44, m_t 3.6e-16 / 3.6e-16 / 1.53, S_t 3.2e-16 / 3.6e-16 / 1.59, lam_t 3.5e-15 / 5.0e-15 / 2.24,
                   Psi_t 1.4e-13 / 1.4e-13 / 2.09, dEsde_dm 4.9e-15 / 9.9e-15 / 2.74, dEsde_dS 9.7e-14 / 1.4e-13 / 2.28
  lane pass        F 3.8e-16 / 5.7e-16 / 5.13, gLa 5.3e-14 / 5.3e-14 / 3.16, gLb 3.0e-14 / 2.8e-14 / 2.76, E_sde 2.5e-15 / 3.3e-15 / 9.53,
                   E_obs 4.8e-16 / 5.5e-16 / 1.97, m_t 3.1e-16 / 3.1e-16 / 1.57, S_t 2.4e-16 / 2.4e-16 / 1.00
(the three figures of a row are each the worst of their kind, not of one case).  The module takes 15 s.
"""
import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from test_gpu_edge_cases import fused_grad_switch, gpu_context, helper_switch
from test_kernel_paths import expected_plan
from test_stepper_rounding_cpu import (COVER_CASES, DT, FUSED_QUANTITIES, LANE_PASS_CASES, OP_CASES, OP_QUANTITIES, PATH_CASES, UNIT, bound,
                                       case_id, checked, fused_problem, fused_reference, fused_x, ld_rel_err, op_problem, op_reference,
                                       op_shared, ratio, resolve_batch)

pytestmark = pytest.mark.gpu
WORST = {}                 # (family, quantity) -> the worst ratio err_k / max(err_o, 2^-53) of this process's run
MATRIX_KEYS = ("st", "psit", "dEsde_ds", "Edf")


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _flags(name):
    return getattr(_lib, name) if name else 0


def psi_recovery_term(p, x, psi_ref):
    """Where the plan has store_q, the backward kernel leaves Q''_t = s A_t - 2 Psi_t (s = 1 / sigma^2) where Psi_t would be, and
    vgpa_fetch recovers Psi_t = (s A_t - Q''_t) / 2.  Forming Q''_t and taking the difference again are two roundings, each of at most
    2^-53 relative to a number of the size of s A_t -- not of Psi_t -- so in the norm of the bound Psi_t gains
    2 * 2^-53 * max|s A_t| / max|Psi_t| (the two roundings test_kernel_paths.check_all names); halving is exact."""
    a, _ = p.split(x)
    s = 1.0 / p.sigma[0, 0]
    return 2.0 * UNIT * float(np.max(np.abs(s * a))) / float(np.max(np.abs(np.asarray(psi_ref, dtype=float))))


def compare(tag, family, got, ext, orc, names, extra=None):
    """One line per compared problem: for every quantity  name err_o/err_k/ratio  (ratio = err_k / max(err_o, 2^-53); a `+term` behind it
    is the recovery term its bound gained).  The quantities over their bound are returned."""
    fails, line = [], []
    for q in names:
        err_o, err_k = ld_rel_err(orc[q], ext[q]), ld_rel_err(np.reshape(got[q], np.shape(ext[q])), ext[q])
        more = (extra or {}).get(q, 0.0)
        lim = bound(err_o, more)
        rat = ratio(err_k, err_o)
        line.append(f"{q} {err_o:.1e}/{err_k:.1e}/{rat:.2f}" + (f"+{more:.1e}" if more else ""))
        WORST[(family, q)] = max(WORST.get((family, q), 0.0), rat)
        if not err_k <= lim:
            fails.append((tag, q, err_o, err_k, lim))
    print(tag, " ".join(line))
    return fails


# ---- operator level ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", OP_CASES, ids=case_id)
def test_operator_level_steppers(c, monkeypatch):
    """Context("NONE").solve_fwd / solve_bwd on arbitrary inputs, benign and stiff, all six stepper families: every problem of the context
    has its own A_t; the first, the last and those next to 63 | 64 are compared in m_t, S_t, lam_t and Psi_t."""
    if c.env:
        monkeypatch.setenv("VGPA_ODE_KERNEL", c.env)
    n_cu = _n_cu()
    batch = resolve_batch(c, n_cu)
    m0, s0, sigma = op_shared(c)
    a, b, gm, gs, jm, js = (np.stack(v) for v in zip(*(op_problem(c, k) for k in range(batch))))
    ctx = va.Context("NONE", c.method, c.d, c.n_pts, DT, sigma=sigma, batch=batch, flags=_flags(c.flag))
    plan = ctx.plan()
    want = expected_plan("NONE", c.d, c.method, batch, _flags(c.flag), "nonsym" if c.nonsym and c.d > 1 else "dense", n_cu, n_pts=c.n_pts,
                         ode_kernel=c.env, fused_grad=fused_grad_switch(), helpers=helper_switch())
    stepper = {"pe": "mfma", "sym": "mfma"}.get(c.family, c.family)
    assert plan["fwd"] == plan["bwd"] == stepper, plan
    assert {k: plan[k] for k in ("fwd", "bwd", "sym_units", "launch_sym_units", "helper_roles")} == \
        {k: want[k] for k in ("fwd", "bwd", "sym_units", "launch_sym_units", "helper_roles")}, (plan, want)
    if stepper == "mfma":
        assert plan["sym_units"] == plan["launch_sym_units"] == (c.family == "sym"), plan
    if batch > n_cu and helper_switch() is None:
        assert plan["helper_roles"] == 0                   # (more problems than compute units: the helper roles go away)
    assert not ctx.streaming       # (VGPA_FLAG_STREAM_LARGE_D chunks the FUSED sweep only -- test_every_other_fused_path[streamed-...]; here the flag must change nothing)
    mt, st = ctx.solve_fwd(a, b, m0, s0, sigma)
    lam, psi = ctx.solve_bwd(a, gm, gs, jm, js)
    ctx.close()
    got = {q: np.reshape(v, (batch,) + v.shape[-(2 + (q in MATRIX_KEYS)):]) for q, v in zip(OP_QUANTITIES, (mt, st, lam, psi))}
    fails = []
    for k in checked(batch):
        ext, orc = op_reference(c, k)
        fails += compare(f"[op {case_id(c)}] k={k}", c.family, {q: got[q][k] for q in OP_QUANTITIES}, ext, orc, OP_QUANTITIES)
    assert not fails, fails


# ---- fused level ------------------------------------------------------------------------------------------------------------

def run_fused(c, names, fetched):
    """One context of the case: the plan against DESIGN.md's table (expected_plan), the sweep, the fetches; returns what the checked
    problems need.  `fetched`: the vgpa_fetch keys among `names`."""
    p, _ = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    n, d, batch, flags = c.n_pts, c.d, c.batch, _flags(c.flag)
    ctx = gpu_context(p, batch=batch, flags=flags)
    plan = ctx.plan()
    assert plan == expected_plan(c.model, d, c.method, batch, flags, c.sigma, _n_cu(), n_pts=n, fused_grad=fused_grad_switch(),
                                 helpers=helper_switch()), plan
    if c.flag == "FLAG_STREAM_LARGE_D":
        ctx.set_option(_lib.OPT_LD_CHUNK, STREAM_CHUNK)
    xb = np.stack([fused_x(c, k) for k in range(batch)])
    f, g = ctx.sweep(xb if batch > 1 else xb[0])
    res = ctx.resident()
    got = dict(F=np.atleast_1d(f), g=np.reshape(g, (batch, -1)), streaming=ctx.streaming)
    for q in fetched:
        got[q] = np.reshape(ctx.fetch(q), (batch, n) + ((d, d) if q in MATRIX_KEYS else (d,)))
    _, es, eo = ctx.energy_parts()
    got["Esde"], got["Eobs"] = np.atleast_1d(es), np.atleast_1d(eo)
    ctx.close()
    return p, plan, res, got


def check_fused(c, p, plan, got, names):
    fails = []
    k_a = c.n_pts * c.d * c.d
    for k in checked(c.batch):
        ext, orc = fused_reference(c, k)
        mine = {q: got[q][k] for q in names if q not in ("gLa", "gLb")}
        mine["gLa"], mine["gLb"] = got["g"][k][:k_a], got["g"][k][k_a:]
        extra = {"psit": psi_recovery_term(p, fused_x(c, k), ext["psit"])} if plan["store_q"] and "psit" in names else None
        fails += compare(f"[fused {case_id(c)}] k={k}", c.family, mine, ext, orc, names, extra)
    assert not fails, fails


FETCHED = ("mt", "st", "lamt", "psit", "dEsde_dm", "dEsde_ds")
STREAM_CHUNK = 4                       # grid points per chunk of the time-chunked sweep: 9 points are two chunks and a ragged third
STREAMED_QUANTITIES = ("F", "gLa", "gLb", "Esde", "Eobs", "mt", "st", "lamt")       # (Psi_t and dEsde_dS live in chunk buffers only)


@pytest.mark.parametrize("c", COVER_CASES, ids=case_id)
def test_isotropic_cover_kernels(c):
    """Lorenz-96, Sigma = 3.5 I, D = 33, 36, 37, 40, RK2 and RK4: the forward cover kernel (packed S_t), k_energy_l96_r (packed dEsde_dS),
    the backward cover kernel (Q''_t; RK4 from 64 problems on: the gradient waves), k_grad_mfma_q, the unpack and Psi-recovery kernels
    of vgpa_fetch -- benign, stiff and near the optimum, on both sides of 64 problems."""
    p, plan, res, got = run_fused(c, FUSED_QUANTITIES, FETCHED)
    fused = c.method == "rk4" and fused_grad_switch() != "0" and (c.batch >= 64 or fused_grad_switch() == "1")
    assert plan["fwd"] == plan["bwd"] == "mfma" and plan["sym_units"] and plan["bwd_upper"] and plan["store_q"] and plan["packed"], plan
    assert plan["grad_in_bwd_now"] == fused, plan
    assert res["cached"] and res["S"] == "packed" and res["dEs"] == "packed" and res["bwd"] == ("none" if fused else "q"), res
    check_fused(c, p, plan, got, FUSED_QUANTITIES)


@pytest.mark.parametrize("c", PATH_CASES, ids=case_id)
def test_every_other_fused_path(c):
    """One case near the optimum and one stiff case for: the role-specialised steppers (D = 12), VGPA_FLAG_SYM_UNITS (D = 24), the
    symmetric units (D = 52), VGPA_FLAG_KEEP_PSI (D = 40), a diagonal Sigma (D = 40: the upper triangle of dEsde_dS), the generic
    steppers (D = 12), the resident sweep above D = 64 (D = 72) and its time-chunked form (D = 72, chunks of 4 grid points: what it
    still keeps is compared)."""
    names = STREAMED_QUANTITIES if c.family == "streamed" else FUSED_QUANTITIES
    p, plan, res, got = run_fused(c, names, [q for q in FETCHED if q in names])
    claims = {"pe": dict(fwd="mfma", bwd="mfma", sym_units=False, launch_sym_units=False),
              "sym_flag": dict(fwd="mfma", bwd="mfma", sym_units=True, bwd_upper=True, store_q=False),
              "sym": dict(fwd="mfma", bwd="mfma", sym_units=True, bwd_upper=True, store_q=False),
              "keep_psi": dict(fwd="mfma", bwd="mfma", sym_units=True, bwd_upper=False, store_q=False, packed=False),
              "upper": dict(fwd="mfma", bwd="mfma", sym_units=True, bwd_upper=True, store_q=False, packed=False),
              "generic": dict(fwd="generic", bwd="generic"), "large_d": dict(fwd="large_d", bwd="large_d"),
              "streamed": dict(fwd="large_d", bwd="large_d")}[c.family]
    assert {k: plan[k] for k in claims} == claims, plan
    assert got["streaming"] == (c.family == "streamed") and res["cached"], res
    if c.family != "streamed":
        assert (res["S"], res["dEs"], res["bwd"]) == ("whole", "upper" if plan["bwd_upper"] else "whole", "psi"), res
    check_fused(c, p, plan, got, names)


LANE_QUANTITIES = ("F", "gLa", "gLb", "Esde", "Eobs", "mt", "st")


@pytest.mark.parametrize("c", LANE_PASS_CASES, ids=case_id)
def test_fused_lane_pass(c):
    """OU, double well (Euler and RK4, one problem and 70) and Lorenz-63 (all four methods, 520 problems): the fused lane pass, whose
    backward recursion and gradient exist nowhere else (vgpa_fetch materialises lam_t and Psi_t with the separate kernels, so they are
    not compared here) -- F, the gradient, E_sde, E_obs, m_t and S_t of problems 0, 63, 64 and the last; benign and near the optimum."""
    p, plan, res, got = run_fused(c, LANE_QUANTITIES, ("mt", "st"))
    assert plan["fwd"] == plan["bwd"] == "lane" and plan["lane_pass"], plan
    assert res["cached"] and res["moments"] == "time_major" and res["bwd"] == "none", res
    check_fused(c, p, plan, got, LANE_QUANTITIES)


def test_worst_ratios_of_the_module():
    """The worst ratio err_k / max(err_o, 2^-53) per family and quantity over the cases above that ran in this process (after them in
    file order), printed for the log; FACTOR bounds each one except Psi_t where the recovery term was added."""
    for family in dict.fromkeys(f for f, _ in WORST):
        print(f"WORST [{family}]", " ".join(f"{q}={r:.2f}" for (f, q), r in WORST.items() if f == family))
