"""
GPU suite (-m gpu): the forward fragment-cover steppers (33 <= D <= 40; k_ode_sym, ode_sym_impl.h) compute the mean recursion's A_t v on
the matrix cores -- one more chain of products on a row-side fragment the wave holds anyway, against the stage vector as a column-side
fragment; the lanes of column 0 of the blocks named by kCoverVecBlocks publish the rows.  What can go wrong there and nowhere else:
a row block served by the wrong wave, block or lane; a k-pair of the vector fragment that is off (the zero-padded tail at D = 33, 37);
the vector update in the product waves drifting from the one the helper waves send to HBM.

  * m_t and S_t of Context("NONE").solve_fwd against the longdouble restatement of the recursion with the fp64 oracle's own error as the
    yardstick -- the bound of test_stepper_rounding.py (test_stepper_rounding_cpu.bound), imported, not restated -- for D = 33, 37, 39, 40,
    Np = 3, 6, 14, the four steppers, batches of 1 and 3, arbitrary (non-symmetric) A_t;
  * an A_t with a single non-zero row or column and a b_t with a single one, for every row block 0 ... 9;
  * the three role sets (VGPA_SYM_HELPERS = 0 / 1 / 2, child processes) and the plan's own choice, at D = 39 and one problem more than the
    device has compute units: identical in every bit, and the set without helpers against the same bound.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import helper_switch
from test_stepper_rounding_cpu import DT, METHODS, bound, ld_rel_err, ratio

pytestmark = pytest.mark.gpu

DIMS = (33, 37, 39, 40)                  # NB = 9 (33) and 10; 33 and 37: three padded rows, 39: one, 40: none
GRIDS = (3, 6, 14)
ROLE_D, ROLE_NPTS = 39, 6


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def shared(d):
    """(m0, s0, Sigma) of every problem at this D"""
    rng = np.random.default_rng([d, 7])
    return 8.0 + rng.standard_normal(d), 0.2 * np.eye(d), np.diag(3.0 + rng.random(d))


@functools.lru_cache(maxsize=None)
def dense_problem(d, n_pts, k):
    """problem k: a decaying drift with an arbitrary, non-symmetric perturbation of every entry"""
    rng = np.random.default_rng([d, n_pts, k, 11])
    a = 8.0 * np.eye(d) + 0.5 * rng.standard_normal((n_pts, d, d))
    b = 8.0 * shared(d)[0] + rng.standard_normal((n_pts, d))
    return a, b


@functools.lru_cache(maxsize=None)
def reference(method, d, a_key, maker):
    """(restatement, oracle) of one problem as (m_t, S_t) each: computed once per session and shared"""
    a, b = maker(*a_key)
    m0, s0, sigma = shared(d)
    return xr.solve_fwd(method, DT, a, b, m0, s0, sigma), vo.solve_fwd(method, DT, False, a, b, m0, s0, sigma)


def held(tag, got_m, got_s, ext, orc):
    """err_k <= bound(err_o) for m_t and S_t; every figure is printed before it is asserted"""
    fails = []
    for name, got, e, o in (("m_t", got_m, ext[0], orc[0]), ("S_t", got_s, ext[1], orc[1])):
        err_o, err_k = ld_rel_err(o, e), ld_rel_err(np.reshape(got, np.shape(e)), e)
        print(f"{tag} {name}: err_o={err_o:.2e} err_k={err_k:.2e} ratio={ratio(err_k, err_o):.2f}")
        if not err_k <= bound(err_o):
            fails.append((tag, name, err_o, err_k, bound(err_o)))
    return fails


def solve(d, method, n_pts, problems):
    batch = len(problems)
    m0, s0, sigma = shared(d)
    a, b = (np.stack(v) for v in zip(*problems))
    ctx = va.Context("NONE", method, d, n_pts, DT, sigma=sigma, batch=batch)
    plan = ctx.plan()
    assert plan["fwd"] == "mfma" and plan["sym_units"] and plan["launch_sym_units"], plan
    roles = helper_switch()
    assert plan["helper_roles"] == ((2 if batch <= _n_cu() else 0) if roles is None else int(roles)), plan
    mt, st = ctx.solve_fwd(a, b, m0, s0, sigma)
    ctx.close()
    return np.reshape(mt, (batch, n_pts, d)), np.reshape(st, (batch, n_pts, d, d))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("d", DIMS)
def test_forward_moments_against_the_oracle(d, method, batch):
    fails = []
    for n_pts in GRIDS:
        mt, st = solve(d, method, n_pts, [dense_problem(d, n_pts, k) for k in range(batch)])
        for k in sorted({0, batch - 1}):
            ext, orc = reference(method, d, (d, n_pts, k), dense_problem)
            fails += held(f"[D={d} {method} Np={n_pts} B={batch} k={k}]", mt[k], st[k], ext, orc)
    assert not fails, fails


@functools.lru_cache(maxsize=None)
def one_line_problem(d, block, column):
    """A_t = ONE non-zero row (or column) inside row block `block`; b_t = one entry, in the same row block"""
    n_pts = 4
    rng = np.random.default_rng([d, block, int(column), 13])
    r = min(4 * block + 2, d - 1)
    a = np.zeros((n_pts, d, d))
    line = 2.0 + rng.random((n_pts, d))
    if column:
        a[:, :, r] = line
    else:
        a[:, r, :] = line
    b = np.zeros((n_pts, d))
    b[:, min(4 * block + 1, d - 1)] = 1.0
    return a, b


@pytest.mark.parametrize("column", [False, True], ids=["row", "column"])
@pytest.mark.parametrize("block", range(10))
def test_single_row_or_column_in_every_row_block(block, column):
    """The row of A_t m_t that is not zero (row: one; column: every row takes m_r) lands where it belongs, for every row block and both
    block counts (D = 37: NB = 10 with a padded last block; D = 33: NB = 9, block 9 is all padding and the case moves to the last row)."""
    fails = []
    for d, method in ((40, "rk4"), (37, "euler"), (33, "heun")):
        mt, st = solve(d, method, 4, [one_line_problem(d, block, column)])
        ext, orc = reference(method, d, (d, block, column), one_line_problem)
        fails += held(f"[D={d} {method} block={block} {'column' if column else 'row'}]", mt[0], st[0], ext, orc)
        a, b = one_line_problem(d, block, column)
        if not column:                   # rows of m_t that neither A_t nor b_t touches stay at m0, to the bit
            r, rb = min(4 * block + 2, d - 1), min(4 * block + 1, d - 1)
            still = [i for i in range(d) if i not in (r, rb)]
            assert np.array_equal(mt[0][:, still], np.broadcast_to(shared(d)[0][still], (4, len(still)))), (d, block)
    assert not fails, fails


def test_role_sets_agree_bit_for_bit_and_with_the_oracle():
    """D = 39, one problem more than the device has compute units (where the plan itself takes the kernels without helpers), every stepper:
    VGPA_SYM_HELPERS = 0 / 1 / 2 and the plan's own choice give the same bits of m_t and S_t for the first and the last problem."""
    batch = _n_cu() + 1
    code = (
        "import sys, json, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "import test_vector_on_matrix_cores as t\n"
        "out = {}\n"
        "for method in t.METHODS:\n"
        "    mt, st = t.solve(%d, method, %d, [t.dense_problem(%d, %d, k %% 5) for k in range(%d)])\n"
        "    out[method] = {'m': mt[[0, -1]].ravel().tolist(), 's': st[[0, -1]].ravel().tolist()}\n"
        "print(json.dumps(out))\n" % (os.path.dirname(__file__), os.path.dirname(os.path.dirname(os.path.abspath(__file__))), ROLE_D, ROLE_NPTS, ROLE_D, ROLE_NPTS, batch))
    outs = {}
    for roles in ("0", "1", "2", None):
        env = dict(os.environ)
        env.pop("VGPA_SYM_HELPERS", None)
        if roles is not None:
            env["VGPA_SYM_HELPERS"] = roles
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[roles] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for roles in ("1", "2", None):
        for method in METHODS:
            assert outs[roles][method] == outs["0"][method], (roles, method)
    fails = []
    for method in METHODS:
        m = np.reshape(outs["0"][method]["m"], (2, ROLE_NPTS, ROLE_D))
        s = np.reshape(outs["0"][method]["s"], (2, ROLE_NPTS, ROLE_D, ROLE_D))
        for i, k in enumerate((0, (batch - 1) % 5)):
            ext, orc = reference(method, ROLE_D, (ROLE_D, ROLE_NPTS, k), dense_problem)
            fails += held(f"[roles=0 {method} k={k}]", m[i], s[i], ext, orc)
    assert not fails, fails
