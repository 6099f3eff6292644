"""
The fragment-cover steppers (33 <= D <= 40; k_ode_sym, ode_sym_impl.h) keep what is constant per lane over the sweep out of their time
loop: forcing terms masked and negated where they are loaded, operand units masked once per step, table offsets as SGPR base + 32-bit
lane offset, and in the gradient role LDS addresses that hold the buffer's base and out-of-range lanes clamped to valid duplicates
instead of predicated.  These tests run every cover geometry and padding case
on the shortest grids (where a precomputed offset or a per-step increment that is off by one step shows), on every role set (no
helpers, one and two helper roles, the fused backward + gradient kernel), against the numpy oracle, bit for bit across the role sets,
and with a guard band round the caller's gradient buffer.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import TOL, fused_grad_switch, gpu_context, helper_switch, make_problem

pytestmark = pytest.mark.gpu

COVER_DIMS = [33, 36, 37, 39, 40]        # NB = 9 (33, 36) and 10; padded rows 3, 0, 3, 1, 0
SHORT_GRIDS = [2, 3, 5, 14]              # 2: prologue and epilogue, no loop iteration; 3: one iteration
BATCHES = [1, 3, 64]                     # 64: the smallest batch that takes the fused backward + gradient kernel (RK4, Sigma = sigma^2 I)


def batch_of(x, batch, seed=41):
    rng = np.random.default_rng(seed)
    return x[None, :] + 0.02 * rng.standard_normal((batch, x.size))


def expected_helper_roles(batch):
    """Plan::helper_roles as vgpa_api.hip decides it: the switch when it is set, else two roles up to one problem per CU (1, 3, 64 are)."""
    forced = helper_switch()
    return 2 if forced is None else (int(forced) if forced in ("0", "2") else 1)


@pytest.mark.parametrize("sigma", ["diag", "iso"])
@pytest.mark.parametrize("n_pts", SHORT_GRIDS)
@pytest.mark.parametrize("method", ["rk4", "rk2"])
@pytest.mark.parametrize("d", COVER_DIMS)
def test_cover_geometries_short_grids_batches(d, method, n_pts, sigma):
    """F and the gradient of the first, one middle and the last problem against the oracle at TOL, for batches of 1, 3 and 64; the plan
    is asserted first (batch 3: the helper-wave kernels; batch 64 with RK4 and Sigma = sigma^2 I: the fused backward + gradient kernel);
    D = 37: m_t and S_t as the sweep left them resident."""
    p, x = make_problem("L96", d, n_pts, method=method, obs_at=[n_pts - 1] if n_pts < 5 else None, sigma=sigma)
    iso = sigma == "iso"
    for batch in BATCHES:
        xb = batch_of(x, batch)
        ctx = gpu_context(p, batch=batch)
        plan = ctx.plan()
        assert plan["fwd"] == plan["bwd"] == "mfma" and plan["sym_units"]
        assert plan["helper_roles"] == expected_helper_roles(batch)
        fused_possible = iso and method == "rk4" and fused_grad_switch() != "0"
        fused = fused_possible and (batch >= 64 or fused_grad_switch() == "1")
        assert plan["grad_in_bwd_now"] == fused, (batch, plan)
        f, g = ctx.sweep(xb if batch > 1 else xb[0])
        f, g = np.atleast_1d(f), np.asarray(g).reshape(batch, -1)
        for i in sorted({0, batch // 2, batch - 1}):
            f_ref, g_ref, st = vo.sweep(p, xb[i], faithful=False)
            assert abs(f[i] - f_ref) <= TOL * abs(f_ref), (batch, i, f[i], f_ref)
            assert rel_err(g[i], g_ref) < TOL, (batch, i)
            if d == 37 and i == 0:
                mt = np.asarray(ctx.fetch("mt")).reshape((batch,) + np.shape(st["mt"]))
                s_t = np.asarray(ctx.fetch("st")).reshape((batch,) + np.shape(st["st"]))
                assert rel_err(mt[0], st["mt"]) < TOL and rel_err(s_t[0], st["st"]) < TOL, batch
        ctx.close()


VARIANT_CASES = [(d, n, sigma) for d in (33, 37, 40) for n in (3, 14) for sigma in ("diag", "iso")]


def test_role_sets_agree_bit_for_bit():
    """VGPA_SYM_HELPERS = 0 / 1 / 2 (read when a context is created: child processes, each of which prints the helper roles of its plans):
    the masks decided before the loop must not make the roles diverge -- F and the gradient of RK4 sweeps over
    three problems at D = 33, 37, 40, Np = 3 and 14, both forms of Sigma, identical in every bit."""
    code = (
        "import sys, json, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import test_gpu_edge_cases as t\n"
        "out = {}\n"
        "for d, n, sigma in %r:\n"
        "    p, x = t.make_problem('L96', d, n, method='rk4', sigma=sigma)\n"
        "    ctx = t.gpu_context(p, batch=3)\n"
        "    xb = np.stack([x + 0.01 * i for i in range(3)])\n"
        "    f, g = ctx.sweep(xb)\n"
        "    out['%%d %%d %%s' %% (d, n, sigma)] = {'f': [float(v) for v in f], 'g': np.asarray(g).ravel().tolist()}\n"
        "    out.setdefault('helper_roles', []).append(ctx.plan()['helper_roles'])\n"
        "    ctx.close()\n"
        "print(json.dumps(out))\n" % (os.path.dirname(__file__), VARIANT_CASES))
    outs = {}
    for roles in (0, 1, 2):
        env = dict(os.environ)
        env["VGPA_SYM_HELPERS"] = str(roles)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[roles] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert outs[roles].pop("helper_roles") == [roles] * len(VARIANT_CASES), roles
    for key, ref in outs[0].items():
        assert outs[1][key] == ref, key
        assert outs[2][key] == ref, key


class _Inside:
    """A device pointer `offset` doubles into a DeviceBuffer (what sweep_dev takes: an object with .ptr)."""

    def __init__(self, buf, offset):
        self.ptr = ctypes.c_void_p(buf.ptr.value + 8 * int(offset))


@pytest.mark.parametrize("batch", [3, 64])
@pytest.mark.parametrize("d", [33, 37])
def test_guard_band_round_the_gradient_buffer(d, batch):
    """Unpredicated stores may only land on a valid duplicate inside the array: the caller's gradient buffer (which the fused kernel's
    gradient waves and the assembly kernel write in place) sits between two guard bands of a sentinel, which a sweep must leave alone,
    and holds the same bits as a sweep into a plain buffer.  Padded dimensions, RK4, Sigma = sigma^2 I (batch 64: the fused kernel;
    packed S_t and Q'' streams) and the diagonal Sigma.  (S_t, lam_t and Psi_t live in allocations of the library's own, which a test
    cannot put a band round; they are compared with the oracle above.)"""
    guard, sentinel = 4096, -1.2345678e300
    for sigma in ("iso", "diag"):
        p, x = make_problem("L96", d, 6, method="rk4", sigma=sigma)
        xb = batch_of(x, batch)
        ctx = gpu_context(p, batch=batch)
        if sigma == "iso" and batch >= 64 and fused_grad_switch() != "0":
            assert ctx.plan()["grad_in_bwd_now"]
        f_ref, g_ref = ctx.sweep(xb)
        x_buf, g_buf = ctx.alloc(xb.size), ctx.alloc(xb.size + 2 * guard)
        x_buf.upload(xb)
        g_buf.upload(np.full(xb.size + 2 * guard, sentinel))
        f = ctx.sweep_dev(x_buf, _Inside(g_buf, guard))
        got = g_buf.download()
        assert np.array_equal(np.atleast_1d(f), np.atleast_1d(f_ref))
        assert np.all(got[:guard] == sentinel) and np.all(got[guard + xb.size:] == sentinel), sigma
        assert np.array_equal(got[guard:guard + xb.size].reshape(batch, -1), np.asarray(g_ref).reshape(batch, -1)), sigma
        x_buf.free(); g_buf.free()
        ctx.close()
