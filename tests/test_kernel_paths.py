"""
GPU suite (-m gpu): which kernels a context runs (Context.plan, the table of DESIGN.md s.4.0), and the kernels that only
Sigma = sigma^2 I turns on at 33 <= D <= 40 -- the Q'' stream, the packed lower-triangle layouts of S_t and dEsde_dS, the backward
kernel that assembles the gradient on a third set of waves -- against the numpy oracle (lean mode) at every padded dimension, both
Q''-storing steppers, both sides of the batch size that switches the gradient assembly, and grids down to two points.

Every case asserts its plan before it asserts a number: a test that names a kernel must be on it.
"""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_KEEP_PSI, FLAG_MATERIALIZE, FLAG_SYM_UNITS
from conftest import rel_err
from helpers import block_rel_errs
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import fused_grad_switch, gpu_context, helper_switch, make_problem
from test_theta_gradient_cpu import fd_theta_gradient

pytestmark = pytest.mark.gpu
TOL = 1e-9


# ---- the plan table ---------------------------------------------------------------------------------------------------------

def expected_plan(model, d, method, batch, flags=0, sigma="iso", n_cu=256, n_pts=4, ode_kernel=None, fused_grad="", sym_s0=True, helpers=None):
    """DESIGN.md s.4.0, row by row, written from the table and not from make_plan.  sigma: "iso", "diag", "dense" (symmetric) or
    "nonsym"; ode_kernel: VGPA_ODE_KERNEL; fused_grad: the first character of VGPA_FUSED_GRAD; helpers: VGPA_SYM_HELPERS ("0", "1", "2") or
    None when it is not set."""
    sym_inputs = sigma != "nonsym" and sym_s0
    len_x = n_pts * d * (d + 1)

    def stepper():
        if d > 64:
            return "large_d"
        if flags & FLAG_FORCE_GENERIC:
            return "generic"
        if d <= 4 and (d == 1 or batch >= 512) and len_x < 2 ** 22:
            return "lane"
        if 2 <= d <= 4:
            return "wave"
        return "mfma" if sym_inputs else "generic"          # (ode_mfma_supported: every stepper, D <= 64)
    fwd = bwd = stepper()
    sym_units = bool(flags & FLAG_SYM_UNITS) or (batch > n_cu and d <= 40) or (33 <= d <= 40 and ode_kernel != "pe") or 45 <= d <= 64
    lane_pass = fwd == "lane" and model in ("OU", "DW", "L63") and not flags & FLAG_MATERIALIZE and (d == 1 or sym_inputs)
    bwd_upper = sym_units and bwd == "mfma" and not flags & FLAG_KEEP_PSI
    store_q = bwd_upper and sigma == "iso" and model == "L96" and method in ("rk2", "rk4") and 33 <= d <= 40
    packed = store_q and fwd == "mfma"
    grad_in_bwd = packed and method == "rk4" and fused_grad != "0"
    launch_sym_units = sym_units or ode_kernel == "sym"
    helper_roles = 0
    if launch_sym_units and 33 <= d <= 40:
        helper_roles = (2 if batch <= n_cu else 0) if helpers is None else {"0": 0, "1": 1, "2": 2}[helpers]
    return dict(fwd=fwd, bwd=bwd, sym_units=sym_units, launch_sym_units=launch_sym_units, helper_roles=helper_roles, lane_pass=lane_pass,
                bwd_upper=bwd_upper, store_q=store_q, packed=packed, grad_in_bwd=grad_in_bwd,
                grad_in_bwd_now=grad_in_bwd and (batch >= 64 or fused_grad == "1"))


def _sigma_of(form, d):
    if form == "iso":
        return 3.5 * np.eye(d)
    if form == "diag":
        return np.diag(3.0 + np.arange(d) / (2.0 * d))
    s = 3.5 * np.eye(d) + 0.2                                # dense, symmetric, positive definite
    if form == "nonsym":
        s[0, d - 1] += 0.1
    return s


def plan_context(model, d, method, batch, flags=0, sigma="iso", n_pts=4):
    """A context of the given shape on the cheapest valid inputs (no kernel is launched on it)."""
    import vgpa_amd as va
    if model in ("OU", "DW"):
        return va.Context(model, method, 1, n_pts, 0.01, sigma=[[0.8]], theta=[1.0], m0=[0.3], s0=[[0.2]], obs_t=[1], obs_y=[0.5],
                          obs_noise=[[0.04]], batch=batch, flags=flags)
    theta = [10.0, 28.0, 2.667] if model == "L63" else [8.0]
    return va.Context(model, method, d, n_pts, 0.01, sigma=_sigma_of(sigma, d), theta=theta, m0=np.ones(d), s0=0.2 * np.eye(d),
                      obs_t=[1], obs_y=np.ones((1, d)), obs_noise=np.eye(d), batch=batch, flags=flags)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan_rows(n_cu):
    """(model, D, method, batch, flags, Sigma form)"""
    rows = [("OU", 1, "euler", 1, 0, "iso"), ("DW", 1, "rk4", n_cu + 1, 0, "iso"), ("OU", 1, "heun", 600, FLAG_MATERIALIZE, "iso"),
            ("L63", 3, "rk4", 6, 0, "diag"), ("L63", 3, "rk4", 511, 0, "diag"), ("L63", 3, "rk4", 512, 0, "diag"),
            ("L63", 3, "rk4", 512, FLAG_MATERIALIZE, "diag"), ("L63", 3, "rk4", 512, 0, "nonsym"), ("L63", 3, "rk4", 512, FLAG_FORCE_GENERIC, "diag"),
            ("L63", 3, "heun", 2, 0, "dense"), ("L96", 4, "rk4", 1, 0, "iso"), ("L96", 4, "rk4", 512, 0, "iso")]
    for d in (5, 12, 24, 32, 33, 36, 40, 41, 44, 45, 64, 72):
        rows += [("L96", d, "rk4", b, 0, "iso") for b in (1, 63, 64, n_cu, n_cu + 1)]
        rows += [("L96", d, "rk2", 3, 0, form) for form in ("diag", "dense", "nonsym")]
    rows += [("L96", 40, m, b, 0, form) for m in ("euler", "heun", "rk2", "rk4") for b in (3, 64, 511, 512, 513) for form in ("iso", "diag")]
    rows += [("L96", 40, "rk4", b, 0, form) for b in (1, 67) for form in ("dense", "nonsym")]
    for flag in (FLAG_SYM_UNITS, FLAG_KEEP_PSI, FLAG_FORCE_GENERIC, FLAG_MATERIALIZE, FLAG_SYM_UNITS | FLAG_KEEP_PSI):
        rows += [("L96", d, "rk4", b, flag, "iso") for d in (12, 36, 40, 44, 64) for b in (2, 64)]
    return rows


def test_plan_table():
    """DESIGN.md s.4.0 as a test: for every row of (model, D, method, batch, flags, Sigma form) the context's plan is what the table
    says (expected_plan, written from the table).  D = 1 ... 72 over every family boundary (4 | 5, 32 | 33, 40 | 41, 44 | 45, 64 | 72), all
    four steppers at D = 40, batches on both sides of 64, of the CU count and of 512, the four Sigma forms, the four flags that
    enter the plan.  Contexts are created and destroyed; no kernel runs."""
    n_cu = _n_cu()
    rows = plan_rows(n_cu)
    for row in rows:
        model, d, method, batch, flags, form = row
        ctx = plan_context(*row)
        got, want = ctx.plan(), expected_plan(model, d, method, batch, flags, form, n_cu, fused_grad=fused_grad_switch(), helpers=helper_switch())
        res = ctx.resident()
        ctx.close()
        assert got == want, (row, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        assert res == dict(cached=False, moments="row_major", S="whole", dEs="whole", bwd="none", terms=False), row
    assert len(rows) > 150


@pytest.mark.parametrize("family", ["pe", "sym"])
def test_plan_under_the_stepper_family_switch(family, monkeypatch):
    """VGPA_ODE_KERNEL (read at vgpa_create): =pe keeps the role-specialised steppers at 33 <= D <= 40 up to one problem per CU,
    and with them whole matrices and Psi_t; =sym launches the symmetric-unit family at D <= 44 without changing a layout."""
    monkeypatch.setenv("VGPA_ODE_KERNEL", family)
    n_cu = _n_cu()
    for d in (12, 24, 33, 36, 40, 41, 44, 45):
        for batch in (1, 64, n_cu, n_cu + 1):
            for flags in (0, FLAG_SYM_UNITS):
                ctx = plan_context("L96", d, "rk4", batch, flags)
                got = ctx.plan()
                ctx.close()
                want = expected_plan("L96", d, "rk4", batch, flags, "iso", n_cu, ode_kernel=family, fused_grad=fused_grad_switch(), helpers=helper_switch())
                assert got == want, (d, batch, flags, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
    if family == "pe":                 # what the switch is for
        ctx = plan_context("L96", 36, "rk4", 1)
        assert not ctx.plan()["sym_units"] and not ctx.plan()["packed"]
        ctx.close()


def test_plan_under_the_fused_gradient_switch():
    """VGPA_FUSED_GRAD (read once per process: one child process per value): 0 takes the gradient waves away at every batch size,
    1 gives them to every batch size -- where the plan has the packed layouts, and nowhere else."""
    rows = [(d, m, b, fl, form) for d in (32, 33, 40, 41) for m in ("rk4", "rk2") for b in (1, 63, 64) for fl in (0, FLAG_KEEP_PSI)
            for form in ("iso", "diag")]
    code = ("import sys, json\n"
            "sys.path.insert(0, %r)\n"
            "import test_kernel_paths as t\n"
            "out = []\n"
            "for d, m, b, fl, form in %r:\n"
            "    ctx = t.plan_context('L96', d, m, b, fl, form)\n"
            "    out.append(ctx.plan())\n"
            "    ctx.close()\n"
            "print(json.dumps(out))\n" % (os.path.dirname(__file__), rows))
    n_cu = _n_cu()
    for value in ("0", "1"):
        env = dict(os.environ)
        env["VGPA_FUSED_GRAD"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        plans = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1])
        for (d, m, b, fl, form), got in zip(rows, plans):
            want = expected_plan("L96", d, m, b, fl, form, n_cu, fused_grad=value, helpers=helper_switch())
            assert got == want, (value, d, m, b, fl, form, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        assert any(p["grad_in_bwd_now"] for p in plans) == (value == "1")


def test_plan_under_the_helper_switch():
    """VGPA_SYM_HELPERS (read at vgpa_create: one child process per value): 0 / 1 / 2 give the fragment-cover steppers that many helper
    roles at every batch size -- at 33 <= D <= 40, and nowhere else; nothing else of the plan moves.  D on both sides of 32 | 33 and
    40 | 41, batches on both sides of the CU count.  Contexts only: no kernel runs."""
    n_cu = _n_cu()
    rows = [(d, b) for d in (32, 33, 40, 41) for b in (1, n_cu, n_cu + 1)]
    code = ("import sys, json\n"
            "sys.path.insert(0, %r)\n"
            "import test_kernel_paths as t\n"
            "out = []\n"
            "for d, b in %r:\n"
            "    ctx = t.plan_context('L96', d, 'rk4', b)\n"
            "    out.append(ctx.plan())\n"
            "    ctx.close()\n"
            "print(json.dumps(out))\n" % (os.path.dirname(__file__), rows))
    for value in ("0", "1", "2"):
        env = dict(os.environ)
        env["VGPA_SYM_HELPERS"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        plans = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1])
        for (d, b), got in zip(rows, plans):
            want = expected_plan("L96", d, "rk4", b, 0, "iso", n_cu, fused_grad=fused_grad_switch(), helpers=value)
            assert got == want, (value, d, b, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
            assert got["helper_roles"] == (int(value) if d in (33, 40) else 0), (value, d, b)


def test_plan_follows_the_per_problem_inputs():
    """vgpa_set_problem_params / vgpa_set_problem_data make the plan again: per-problem Sigma rows that are all isotropic (each with
    its own sigma_k) keep the packed layouts and the gradient waves, one row that is only diagonal takes them away, and taking the
    rows back restores them; a non-symmetric s0 row sends the sweep to the generic steppers."""
    n_cu, d, batch = _n_cu(), 40, 67
    fused = fused_grad_switch()
    ctx = plan_context("L96", d, "rk4", batch)
    iso, diag = (expected_plan("L96", d, "rk4", batch, 0, form, n_cu, fused_grad=fused, helpers=helper_switch()) for form in ("iso", "diag"))
    assert iso["packed"] and not diag["packed"] and diag["bwd_upper"]
    assert ctx.plan() == iso
    own = np.stack([(3.0 + 0.01 * k) * np.eye(d) for k in range(batch)])
    ctx.set_problem_params(sigma=own)
    assert ctx.plan() == iso                                   # every row sigma_k^2 I
    mixed = own.copy()
    mixed[batch - 1, 5, 5] *= 1.01                             # the last row: diagonal, not isotropic
    ctx.set_problem_params(sigma=mixed)
    assert ctx.plan() == diag
    ctx.set_problem_params(sigma=own)
    assert ctx.plan() == iso
    ctx.set_problem_params(sigma=np.stack([_sigma_of("diag", d)] * batch))
    assert ctx.plan() == diag
    ctx.set_problem_params()                                   # the shared Sigma of the configuration again
    assert ctx.plan() == iso
    s0 = np.stack([0.2 * np.eye(d)] * batch)
    ctx.set_problem_data(s0=s0)
    assert ctx.plan() == iso
    s0[3, 0, 1] += 0.01
    ctx.set_problem_data(s0=s0)
    assert ctx.plan() == expected_plan("L96", d, "rk4", batch, 0, "iso", n_cu, fused_grad=fused, sym_s0=False, helpers=helper_switch())
    assert ctx.plan()["fwd"] == "generic" and not ctx.plan()["packed"]
    ctx.set_problem_data()
    assert ctx.plan() == iso
    ctx.close()


# ---- the isotropic cover-kernel matrix against the oracle -------------------------------------------------------------------

FETCHED = ("mt", "st", "lamt", "psit", "dEsde_dm", "dEsde_ds", "Efx", "Edf")
WORST = {}                 # block -> the worst error of the module's run (printed by the last test of the matrix)


def assert_cover_plan(ctx, method, batch):
    """the plan of a default Lorenz-96 context at 33 <= D <= 40 with Sigma = sigma^2 I: RK2 and RK4 store Q''_t and pack; RK4 assembles
    the gradient in the backward kernel from 64 problems on"""
    plan = ctx.plan()
    fused = method == "rk4" and fused_grad_switch() != "0" and (batch >= 64 or fused_grad_switch() == "1")
    assert plan["fwd"] == plan["bwd"] == "mfma" and plan["sym_units"] and plan["bwd_upper"] and plan["store_q"] and plan["packed"], plan
    assert plan["grad_in_bwd_now"] == fused, plan
    return fused


def check_all(probs, xb, ctx, fused):
    """Every problem of the context against vo.sweep(p_i, x_i, faithful=False): F; gLa and gLb, each relative to its own block; every
    vgpa_fetch key the oracle's state has, each on its own scale; E_sde and E_obs.  The record of the buffers is asserted on the way.
    Returns the worst error per block."""
    batch = len(probs)
    n, d = probs[0].n_pts, probs[0].dim_d
    f, g = ctx.sweep(xb if batch > 1 else xb[0])
    f, g = np.atleast_1d(f), np.reshape(g, (batch, -1))
    res = ctx.resident()
    assert res["cached"] and res["S"] == "packed" and res["dEs"] == "packed" and res["bwd"] == ("none" if fused else "q"), res
    got = {key: np.reshape(ctx.fetch(key), (batch, n, d) + ((d,) if key in ("st", "psit", "dEsde_ds", "Edf") else ())) for key in FETCHED}
    assert ctx.resident()["bwd"] == "psi"                       # (Q''_t -- stored for the fetch behind the gradient waves -- recovered in place)
    e0, es, eo = (np.atleast_1d(v) for v in ctx.energy_parts())
    # unpacked lower triangles come back exactly symmetric; Psi_t recovered from Q''_t = s A_t - 2 Psi_t with a non-symmetric A_t is
    # symmetric to the rounding of the recovery (two roundings of s |A_ij| ~ 2.3 against |Psi_t| ~ 1: the 1e-13 of
    # test_q_stream_of_the_batched_sweeps for the same recovery)
    for key in ("st", "dEsde_ds"):
        assert np.array_equal(got[key], np.swapaxes(got[key], 2, 3)), key
    assert rel_err(np.swapaxes(got["psit"], 2, 3), got["psit"]) < 1e-13
    worst = {}
    for i, p in enumerate(probs):
        f_ref, g_ref, st = vo.sweep(p, xb[i], faithful=False)
        e_la, e_lb = block_rel_errs(g[i], g_ref, n, d)
        errs = {"F": abs(f[i] - f_ref) / abs(f_ref), "gLa": e_la, "gLb": e_lb, "Esde": abs(es[i] - st["Esde"]) / abs(st["Esde"]),
                "Eobs": abs(eo[i] - st["Eobs"]) / abs(st["Eobs"])}
        for key in FETCHED:
            errs[key] = rel_err(got[key][i], np.reshape(st[key], got[key][i].shape))
        for key, e in errs.items():
            worst[key] = max(worst.get(key, 0.0), e)
    return worst


def report_and_assert(tag, worst):
    print(tag, " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    for key, e in worst.items():
        WORST[key] = max(WORST.get(key, 0.0), e)
        assert e < TOL, (tag, key, e)


def batch_of(x, batch, seed):
    return x[None, :] + 0.02 * np.random.default_rng(seed).standard_normal((batch, x.size))


# (D, method, batch, Np, observation indices): every D with both steppers on both sides of 64 problems; every Np with the separate
# assembly (k_grad_mfma_q: RK2, and RK4 below 64 problems) and with the gradient waves (RK4 from 64 on); D = 33, 34, 37, 38 -- an odd
# packed length D (D + 1) / 2, every second grid point 8 bytes off a 16-byte boundary -- with Np >= 3 everywhere; observations at the
# first index, at the last index and inside; batches of 67 leave the last launch round ragged
COVER_CASES = [
    (33, "rk4", 67, 3, [0]), (34, "rk4", 64, 4, [3]), (35, "rk4", 67, 2, [1]), (36, "rk4", 64, 5, [2]),
    (37, "rk4", 67, 6, [0, 5]), (38, "rk4", 64, 9, [4]), (39, "rk4", 67, 24, [2, 7, 12, 17, 22]), (40, "rk4", 64, 4, [1, 2]),
    (33, "rk4", 1, 24, [2, 7, 12, 17, 22]), (34, "rk4", 3, 9, [0, 8]), (35, "rk4", 1, 6, [2]), (36, "rk4", 3, 2, [0]),
    (37, "rk4", 1, 5, [4]), (38, "rk4", 3, 3, [1]), (39, "rk4", 1, 4, [0]), (40, "rk4", 3, 6, [5]),
    (33, "rk2", 64, 5, [1, 3]), (34, "rk2", 67, 3, [2]), (35, "rk2", 64, 4, [0]), (36, "rk2", 67, 9, [2, 7]),
    (37, "rk2", 64, 3, [1]), (38, "rk2", 67, 6, [0, 4]), (39, "rk2", 64, 2, [1]), (40, "rk2", 67, 6, [0, 5]),
    (33, "rk2", 3, 4, [3]), (34, "rk2", 1, 6, [0]), (35, "rk2", 3, 24, [2, 7, 12, 17, 22]), (36, "rk2", 1, 3, [0]),
    (37, "rk2", 3, 9, [8]), (38, "rk2", 1, 5, [2]), (39, "rk2", 3, 2, [0]), (40, "rk2", 1, 5, [0, 4]),
]


def test_cover_cases_meet_the_coverage_conditions():
    """The thinned cross product keeps what it was thinned under (no GPU work: the table alone)."""
    for d in range(33, 41):
        mine = [c for c in COVER_CASES if c[0] == d]
        assert {(c[1], c[2] >= 64) for c in mine} == {(m, big) for m in ("rk2", "rk4") for big in (False, True)}, d
        if d * (d + 1) // 2 % 2:
            assert d in (33, 34, 37, 38) and all(c[3] >= 3 for c in mine), d
    waves = {c[3] for c in COVER_CASES if c[1] == "rk4" and c[2] >= 64}
    separate = {c[3] for c in COVER_CASES if not (c[1] == "rk4" and c[2] >= 64)}
    assert waves == separate == {2, 3, 4, 5, 6, 9, 24}
    assert {c[2] for c in COVER_CASES} == {1, 3, 64, 67}
    assert any(c[4][0] == 0 for c in COVER_CASES) and any(c[4][-1] == c[3] - 1 for c in COVER_CASES)
    assert any(0 < t < c[3] - 1 for c in COVER_CASES for t in c[4])


@pytest.mark.parametrize("d,method,batch,n_pts,obs", COVER_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_isotropic_cover_kernels_against_the_oracle(d, method, batch, n_pts, obs):
    """Lorenz-96, Sigma = 3.5 I, 33 <= D <= 40: forward cover kernel (packed S_t) -> observation kernel -> k_energy_l96_r (packed
    dEsde_dS) -> backward cover kernel (Q''_t; RK4 from 64 problems on: the gradient waves) -> k_grad_mfma_q -> the unpack and
    Psi-recovery kernels of vgpa_fetch.  EVERY problem against the oracle at TOL = 1e-9: F, gLa and gLb each on its own scale, the
    eight state arrays, E_sde, E_obs; S_t and dEsde_dS exactly symmetric.  The plan and the record of the buffers are asserted first.
    Worst values over the 32 cases, measured on an MI355X (profiles/kernel_paths_gputests.log has every case): F 1.3e-16, gLa 2.9e-15,
    gLb 2.7e-15, E_sde 5.7e-16, E_obs 4.1e-16, m_t 3.4e-16, S_t 4.1e-16, lam_t 2.2e-15, Psi_t 5.4e-15, dEsde_dm 5.5e-15,
    dEsde_dS 9.7e-15, <f> 1.5e-15, <df/dx> 5.1e-16."""
    p, x = make_problem("L96", d, n_pts, method=method, obs_at=obs, sigma="iso")
    ctx = gpu_context(p, batch=batch)
    fused = assert_cover_plan(ctx, method, batch)
    worst = check_all([p] * batch, batch_of(x, batch, 100 * d + n_pts), ctx, fused)
    ctx.close()
    report_and_assert(f"cover D={d} {method} B={batch} Np={n_pts} obs={obs}:", worst)


@pytest.mark.parametrize("d,method,batch,n_pts,obs", [(37, "rk4", 67, 5, [0, 3]), (34, "rk2", 3, 6, [5])])
def test_isotropic_rows_with_their_own_sigma(d, method, batch, n_pts, obs):
    """Per-problem Sigma_k = sigma_k^2 I (vgpa_set_problem_params): the packed path stays, and the Q'' kernels take 1 / sigma_k^2 from
    OdeArgs::q_scale_v.  Every problem against the oracle with its own sigma_k, as above.  Measured: gLa 2.5e-15, gLb 2.7e-15,
    Psi_t 2.2e-15, dEsde_dS 6.0e-15, everything else below 4e-15."""
    p, x = make_problem("L96", d, n_pts, method=method, obs_at=obs, sigma="iso")
    probs = [dataclasses.replace(p, sigma=(2.5 + 0.03 * k) * np.eye(d)) for k in range(batch)]
    ctx = gpu_context(p, batch=batch)
    ctx.set_problem_params(sigma=np.stack([q.sigma for q in probs]))
    fused = assert_cover_plan(ctx, method, batch)
    worst = check_all(probs, batch_of(x, batch, 7 * d), ctx, fused)
    ctx.close()
    report_and_assert(f"own sigma D={d} {method} B={batch} Np={n_pts}:", worst)


@pytest.mark.parametrize("batch", [3, 65])
@pytest.mark.parametrize("d", [35, 38])
def test_theta_gradient_behind_the_packed_state(d, batch):
    """vgpa_theta_gradient reads the resident S_t in the layout it is in: packed here, at a padded dimension, behind an F-only
    evaluation (B = 65: no backward recursion has run) and behind a sweep.  Reference: the central difference of the oracle's F in
    theta, exact for the quadratic F is in theta (test_theta_gradient.py); TOL = 1e-9.  Measured: 2.1e-12 (D = 35), 1.2e-11 (D = 38) --
    the rounding of the difference quotient."""
    p, x = make_problem("L96", d, 7, method="rk4", obs_at=[0, 3], sigma="iso")
    xb = batch_of(x, batch, d)
    ctx = gpu_context(p, batch=batch)
    fused = assert_cover_plan(ctx, "rk4", batch)
    ctx.free_energy(xb)
    assert ctx.resident()["S"] == "packed" and ctx.resident()["bwd"] == "none"       # (grad_in_bwd: F needs no recursion)
    g_f = np.asarray(ctx.theta_gradient())
    _, g = ctx.sweep(xb)
    g_s = np.asarray(ctx.theta_gradient())
    assert ctx.resident()["bwd"] == ("none" if fused else "q")
    assert np.array_equal(ctx.gradient(None), g) and np.array_equal(g_f, g_s)         # the cached state survives; the same kernel twice
    ctx.close()
    assert g_f.shape == (batch, 1)
    worst = 0.0
    for k in sorted({0, 1, batch // 2, batch - 1}):
        worst = max(worst, rel_err(g_f[k], fd_theta_gradient(p, xb[k])))
    print(f"theta gradient D={d} B={batch}: worst {worst:.1e}")
    assert worst <= TOL


def test_free_energy_then_gradient_on_the_gradient_waves():
    """The F-only evaluation of a context whose backward kernel assembles the gradient skips the recursion; gradient(None) then
    runs it.  D = 33 (padded, odd packed length), Np = 3: bit-equal to the one-call sweep, as
    test_gradient_waves_of_the_backward_kernel asserts at D = 40."""
    p, x = make_problem("L96", 33, 3, method="rk4", obs_at=[1], sigma="iso")
    batch = 67
    xb = batch_of(x, batch, 3)
    ctx = gpu_context(p, batch=batch)
    fused = assert_cover_plan(ctx, "rk4", batch)
    f, g = ctx.sweep(xb)
    f2 = ctx.free_energy(xb)
    assert ctx.resident()["bwd"] == "none" and ctx.resident()["terms"]
    g2 = ctx.gradient(None)
    assert ctx.resident()["bwd"] == ("none" if fused else "q")
    assert np.array_equal(f2, f) and np.array_equal(g2, g)
    f3 = ctx.free_energy(xb[::-1].copy())
    assert np.array_equal(f3, f[::-1]) and np.array_equal(ctx.gradient(None), g[::-1])
    ctx.close()


def test_worst_errors_of_the_cover_matrix():
    """The worst relative error per block over the cases above that ran in this process (after them in file order), printed for the
    log.  Measured on an MI355X over the 32 + 2 cases (profiles/kernel_paths_gputests.log): F 1.3e-16, gLa 2.9e-15, gLb 2.7e-15,
    E_sde 5.7e-16, E_obs 4.3e-16, m_t 3.4e-16, S_t 4.1e-16, lam_t 2.2e-15, Psi_t 5.4e-15, dEsde_dm 5.5e-15, dEsde_dS 9.7e-15,
    <f> 1.5e-15, <df/dx> 5.1e-16."""
    print("worst over the module:", " ".join(f"{k}={v:.1e}" for k, v in WORST.items()))
    assert all(e < TOL for e in WORST.values())
