"""
GPU suite (-m gpu): phase 5 of k_energy_l96_r on its packed branch -- dE/dS = (c/2) X^T diag(q) X from 16 x 16 tiles of X = L^-1
(v_mfma_f64_16x16x4_f64) and dE/dm = (c/2) X^T delta from the same fragments -- at D = 33, 36, 37, 40: NB = 9 and 10, padded and unpadded
last blocks, a last tile column that reaches past the matrix by 12, 12, 8 and 8 columns.  Np = 9, two problems, the fused sweep, so that
dEsde_dS travels as packed lower triangles (asserted on the plan and on the record of the buffers).

Inputs, per D:
  * "benign": the seeded datasets of helpers.build_problem, one per problem as test_problem_batch._datasets makes them, observed at the
    grid points 2 and 6; cond(S_t) <= 3;
  * "stiff S": the problems of test_l96_energy_conditioning_cpu.theta_inputs (s0 of condition 1e4, dt = 1e-3) at nine grid points, with
    Sigma = 3.5e-4 I in the place of their 1e-4 diag(3 .. 4): only an isotropic Sigma takes the packed layouts.  That cond(S_t) >= 1e3
    holds at every grid point with this Sigma too is asserted here, on the oracle's forward sweep.

What is compared, against the longdouble restatement of the sweep (extended_ref.sweep) with the fp64 oracle's own error as the yardstick:
  * dEsde_dS and dEsde_dm, fetched after the sweep, under the rule of test_l96_energy_conditioning.py (its _assert_close: err_k <=
    max(32 err_o, 64 D 2^-53) in conftest.rel_err's norm; it prints err_o, err_k and their ratio per quantity);
  * gLa and gLb of the same sweeps under the bound of test_stepper_rounding.py's fused level (its compare);
  * the unpacked dEsde_dS equals its transpose bit for bit (the store mask of the tiles: col <= row, row < D);
  * a not-positive-definite S_0 in one problem still raises LinAlgError naming that problem (the kernel's early return stands in
    front of phase 5).

Measured on an MI355X (twelve cases, 2 s): worst err_k / err_o 1.86 in dEsde_dS / dEsde_dm (stiff S: err_o 4e-14 ... 1.2e-13), 2.06 in
gLa / gLb; the kernel of the parent commit (4 x 4 x 4 units throughout, a separate dE/dm loop) was run on the stiff-S cases and passes them too.
"""
import dataclasses
import functools

import numpy as np
import pytest

import extended_ref as xr
from oracle import vgpa_oracle as vo
from test_l96_energy_conditioning import _assert_close, _theta_context
from test_l96_energy_conditioning_cpu import bad_s0, bad_set, theta_inputs
from helpers import SEED, build_problem
from test_problem_batch import _context, _oracle_problem
from test_stepper_rounding import compare

pytestmark = pytest.mark.gpu

DIMS = (33, 36, 37, 40)
N_PTS, NB = 9, 2
OBS_AT = (2, 6)
KINDS = ("benign", "stiff_s")
COND = {"benign": 1e2, "stiff_s": 1e4}          # the row of test_l96_energy_conditioning.FACTOR each kind is held to (cond(S_t) <= 3 | >= 1e3)


@functools.lru_cache(maxsize=None)
def _inputs(kind, d):
    """(base dataset or None, oracle problems, x per problem): once per session"""
    if kind == "benign":       # (test_problem_batch._datasets with explicit observation indices: nine grid points hold no equidistant one)
        base = [build_problem("L96", "rk4", (N_PTS - 1) * 0.01, dim_d=d, seed=SEED + j, obs_at=OBS_AT) for j in range(NB)]
        rng = np.random.default_rng(7)
        probs, xs = [], []
        for k, p in enumerate(base):
            probs.append(_oracle_problem(p, "L96", "rk4", m0=np.asarray(p["m0"], dtype=float) + 0.01 * k,
                                         s0=np.asarray(p["s0"], dtype=float) * (1.0 + 0.05 * k)))
            x0 = p["init"]()
            xs.append(x0 + 1e-3 * rng.standard_normal(x0.size))
        return base[0], probs, np.stack(xs)
    probs, xs = theta_inputs(d, NB, n_pts=N_PTS)
    return None, [dataclasses.replace(p, sigma=3.5e-4 * np.eye(d)) for p in probs], xs


@functools.lru_cache(maxsize=None)
def _reference(kind, d, k):
    """(restatement, oracle) of problem k: dicts over dEsde_dm, dEsde_dS, gLa, gLb"""
    _, probs, xs = _inputs(kind, d)
    p, x = probs[k], xs[k]
    n_a = p.n_pts * d * d
    f, gla, glb, state = xr.sweep(p, x, float(np.asarray(vo.kl0(p))))
    _, g_o, st_o = vo.sweep(p, x, faithful=False)
    ext = dict(dEsde_dm=state["dEsde_dm"], dEsde_dS=state["dEsde_ds"], gLa=gla, gLb=glb)
    orc = dict(dEsde_dm=st_o["dEsde_dm"], dEsde_dS=st_o["dEsde_ds"], gLa=g_o[:n_a], gLb=g_o[n_a:])
    return ext, orc


def _open(kind, d):
    base, probs, _ = _inputs(kind, d)
    ctx = _context(base, probs, NB) if kind == "benign" else _theta_context(probs, NB)
    plan = ctx.plan()
    assert plan["packed"] and plan["store_q"] and plan["fwd"] == plan["bwd"] == "mfma", plan
    return ctx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_packed_dEsde_from_tiles(d, kind):
    _, probs, xs = _inputs(kind, d)
    conds = [np.linalg.cond(s) for p, x in zip(probs, xs) for s in vo.solve_fwd(p.method, p.dt, False, *p.split(x), p.m0, p.s0, p.sigma)[1]]
    print(f"[tile {kind}] D={d}: cond(S_t) {min(conds):.1e} .. {max(conds):.1e}")
    assert (max(conds) <= 3.0) if kind == "benign" else (min(conds) >= 1e3)
    ctx = _open(kind, d)
    _, g = ctx.sweep(xs)
    res = ctx.resident()
    assert res["S"] == "packed" and res["dEs"] == "packed", res
    g = np.reshape(g, (NB, -1))
    dm = np.reshape(ctx.fetch("dEsde_dm"), (NB, N_PTS, d))
    ds = np.reshape(ctx.fetch("dEsde_ds"), (NB, N_PTS, d, d))
    ctx.close()
    assert np.all(np.isfinite(dm)) and np.all(np.isfinite(ds))
    assert np.array_equal(ds, np.swapaxes(ds, -1, -2))
    fails = []
    n_a = N_PTS * d * d
    for k in range(NB):
        ext, orc = _reference(kind, d, k)
        tag = f"[tile {kind}] D={d} k={k}"
        _assert_close(tag, d, COND[kind], dict(dEsde_dm=dm[k], dEsde_dS=ds[k]), ext, orc, ("dEsde_dm", "dEsde_dS"))
        fails += compare(tag, "tile_syrk", dict(gLa=g[k][:n_a], gLb=g[k][n_a:]), ext, orc, ("gLa", "gLb"))
    assert not fails, fails


@pytest.mark.parametrize("d", DIMS)
def test_not_positive_definite_still_ends_before_phase_5(d):
    base, probs, xs = _inputs("benign", d)
    k = NB - 1
    s0 = bad_s0(probs[k], k)
    assert bad_set(probs[k], xs[k], s0=s0) == {0}
    ctx = _open("benign", d)
    m = probs[0].obs_t.size
    ctx.set_problem_data(obs_y=np.stack([np.reshape(q.obs_y, (m, d)) for q in probs]), m0=np.stack([q.m0 for q in probs]),
                         s0=np.stack([np.asarray(q.s0, dtype=float) if j != k else s0 for j, q in enumerate(probs)]))
    with pytest.raises(np.linalg.LinAlgError, match=rf"problem {k}:"):
        ctx.sweep(xs)
    ctx.close()
