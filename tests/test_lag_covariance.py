"""
vgpa_lag_covariance on the device (lag_cov.hip): the two-time covariance K(k, s) = Phi(k, s) S_s of the posterior process
and its propagator Phi(k, s), held to rounding error against the references of test_lag_covariance_cpu.py (which says what they are, what the
case table covers and where the statistical bound comes from).

Rounding.  Per (case, problem, anchor, kept k >= s): err_k <= 32 max(err_o, 2^-53), both errors relative in the max norm of that D x D block and
measured against the longdouble restatement; err_o is the fp64 oracle restatement's.  The covariance kind starts its references from the S_s
the device holds (vgpa_fetch): the row k = s is that matrix bit for bit, and the test is of the recursion behind it.
Exact properties.  Row k = s is the fetched S_s or I; an anchor's block is the same alone or among others; a problem's block the same alone
or in a batch; the kept rows do not depend on the stride; the rows before the anchor are zero; the cached state is untouched.
"""
import os

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from test_gpu_edge_cases import gpu_context, make_problem
from test_lag_covariance_cpu import (CASES, KINDS, STAT_ANCHORS, STAT_MODELS, STAT_PATHS, STAT_SEED, anchors_of, block_errors, case_id, case_problem,
                                     case_reference, case_x, check_sampler_link, stat_problem)
from test_sample_paths_cpu import em_moments
from helpers import SEED, build_problem
from test_stepper_rounding_cpu import bound, checked, ratio

pytestmark = pytest.mark.gpu

WORST = {}                 # kind -> the worst ratio err_k / max(err_o, 2^-53) of this process's run


def fetched_st(ctx, c):
    return np.asarray(ctx.fetch("st")).reshape(c.batch, c.n_pts, c.d, c.d)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_rounding_and_exact_rows(c):
    p, _ = case_problem(c)
    xs = np.stack([case_x(c, k) for k in range(c.batch)])
    anchors = anchors_of(c)
    ctx = gpu_context(p, batch=c.batch)
    ctx.free_energy(xs)
    st = fetched_st(ctx, c)
    kept = np.arange(0, c.n_pts, c.stride)
    for kind in KINDS:
        res = ctx.lag_covariance(anchors, kind, stride=c.stride)
        assert res.values.shape == (c.batch, len(anchors), kept.size, c.d, c.d)
        assert list(res.anchors) == anchors and list(res.grid) == list(kept) and res.kind == kind
        for k in checked(c.batch):
            for i, s in enumerate(anchors):
                got = res.values[k, i]
                assert not np.any(got[kept < s]), (kind, k, s)                                # rows before the anchor
                if s % c.stride == 0:                                                         # row k = s, exactly
                    assert np.array_equal(got[s // c.stride], st[k, s] if kind == "covariance" else np.eye(c.d)), (kind, k, s)
                ext, orc = case_reference(c, k, s, kind, st[k])
                err_o, err_k = block_errors(orc, ext, s, c.stride), block_errors(got, ext, s, c.stride)
                for j in err_k:
                    print(f"{case_id(c)} {kind} problem {k} anchor {s} k {j}: err_k {err_k[j]:.3e} err_o {err_o[j]:.3e}")
                    WORST[kind] = max(WORST.get(kind, 0.0), ratio(err_k[j], err_o[j]))
                    assert err_k[j] <= bound(err_o[j]), (kind, k, s, j, err_k[j], err_o[j])
    ctx.close()


def _context_with_state(model, d, n_pts, method, batch, seed=23, sigma="diag"):
    p, x = make_problem(model, d, n_pts, method=method, sigma=sigma)
    rng = np.random.default_rng(seed)
    xs = np.stack([x + 0.02 * rng.standard_normal(x.size) for _ in range(batch)])
    ctx = gpu_context(p, batch=batch)
    ctx.free_energy(xs)
    return p, xs, ctx


EXACT = [("OU", 1, "heun", 9), ("DW", 1, "rk4", 9), ("L63", 3, "rk4", 9), ("L96", 5, "euler", 9), ("L96", 17, "rk2", 9), ("L96", 40, "rk4", 9),
         ("L96", 64, "heun", 9)]


@pytest.mark.parametrize("model,d,method,n_pts", EXACT, ids=lambda v: str(v))
def test_an_anchor_does_not_see_the_other_anchors_nor_the_batch_nor_the_stride(model, d, method, n_pts):
    p, xs, ctx = _context_with_state(model, d, n_pts, method, 3)
    every = list(range(n_pts))
    for kind in KINDS:
        full = ctx.lag_covariance(every, kind).values                       # (3, Np, Np, D, D)
        for s in (0, 4, n_pts - 1):
            alone = ctx.lag_covariance([s], kind).values
            assert np.array_equal(alone[:, 0], full[:, s]), (kind, s)       # alone or among others
        pair = ctx.lag_covariance([1, 6], kind).values
        assert np.array_equal(pair[:, 0], full[:, 1]) and np.array_equal(pair[:, 1], full[:, 6]), kind
        for stride in (2, 3):
            strided = ctx.lag_covariance([1, 6], kind, stride=stride).values
            assert np.array_equal(strided, pair[:, :, ::stride]), (kind, stride)      # the stride-3 rows are the stride-1 rows
            assert not np.any(strided[:, 1, :(6 + stride - 1) // stride]), (kind, stride)
    # a problem alone gives what it gives in the batch: its own context, its own x
    for k in (0, 2):
        one = gpu_context(p, batch=1)
        one.free_energy(xs[k])
        for kind in KINDS:
            assert np.array_equal(one.lag_covariance([0, 3], kind, stride=2).values[0], ctx.lag_covariance([0, 3], kind, stride=2).values[k]), (kind, k)
        one.close()
    ctx.close()


LAYOUTS = [("OU", 1, "rk4", 2, "diag", ("time_major", "whole")), ("L63", 3, "rk4", 2, "diag", ("row_major", "whole")),
           ("L63", 3, "heun", 520, "diag", ("time_major", "whole")), ("L96", 12, "rk2", 2, "diag", ("row_major", "whole")),
           ("L96", 40, "rk4", 2, "iso", ("row_major", "packed")), ("L96", 52, "rk4", 1, "diag", ("row_major", "whole"))]


@pytest.mark.parametrize("model,d,method,batch,sigma,layout", LAYOUTS, ids=lambda v: str(v))
def test_the_cached_state_is_untouched(model, d, method, batch, sigma, layout):
    """every layout S_t can be resident in: the lane pass's time-major array (OU; Lorenz-63 from 512 problems), whole matrices, the packed
    lower triangles of the fragment-cover kernels (D = 40, Sigma = sigma^2 I)"""
    n_pts = 9
    p, xs, ctx = _context_with_state(model, d, n_pts, method, batch, sigma=sigma)
    if not (layout[1] == "packed" and os.environ.get("VGPA_ODE_KERNEL") == "pe"):        # (that switch keeps the role-specialised steppers: whole matrices)
        assert (ctx.resident()["moments"], ctx.resident()["S"]) == layout
    grad = np.array(ctx.gradient(None))
    first = ctx.lag_covariance([0, 4], "covariance").values                  # before anything was fetched: the layout the sweep left
    before = {key: np.array(ctx.fetch(key)) for key in ("mt", "st")}
    control = gpu_context(p, batch=batch)                                    # the same evaluation without the call
    control.free_energy(xs)
    for key in before:
        assert np.array_equal(np.array(control.fetch(key)), before[key]), key
    control.close()
    theta = np.array(ctx.theta_gradient())
    parts = np.array(ctx.energy_parts())
    res = ctx.lag_covariance([0, 4], "covariance").values
    phi = ctx.lag_covariance([0, 4], "propagator").values
    assert np.array_equal(res, first)
    st = before["st"].reshape(batch, n_pts, d, d)
    assert np.array_equal(res[:, 0, 0], st[:, 0]) and np.array_equal(res[:, 1, 4], st[:, 4])
    assert np.array_equal(phi[:, 1, 4], np.broadcast_to(np.eye(d), (batch, d, d)))
    assert np.array_equal(np.array(ctx.gradient(None)), grad)
    for key in before:
        assert np.array_equal(np.array(ctx.fetch(key)), before[key]), key
    assert np.array_equal(np.array(ctx.theta_gradient()), theta)
    assert np.array_equal(np.array(ctx.energy_parts()), parts)
    # the cached x is the propagator's: the same bits as with x given, which drops the cache
    assert np.array_equal(ctx.lag_covariance([0, 4], "propagator", x=xs).values, phi)
    with pytest.raises(RuntimeError):
        ctx.gradient(None)
    ctx.close()


@pytest.mark.parametrize("model,d", STAT_MODELS)
def test_empirical_cross_covariance_of_sampled_paths(model, d):
    p, x = stat_problem(model, d)
    ctx = gpu_context(p)
    ctx.free_energy(x)
    paths = ctx.sample_paths("posterior", STAT_PATHS, STAT_SEED)[0]
    res = ctx.lag_covariance(list(STAT_ANCHORS), "propagator")
    phi = {s: res.values[0, i] for i, s in enumerate(STAT_ANCHORS)}
    _, var_em = em_moments(p, x)
    worst = check_sampler_link(paths, phi, var_em)
    print(f"{model} D = {d}: worst deviation {worst:.2f} standard errors")
    ctx.close()


def test_python_layers():
    p, x = make_problem("L96", 12, 9)
    vgp_like = gpu_context(p)
    vgp_like.free_energy(x)
    want = vgp_like.lag_covariance([0, 2], "covariance", stride=2)
    # the covariance kind with an x evaluates free_energy(x) first
    fresh = gpu_context(p)
    got = fresh.lag_covariance([0, 2], "covariance", stride=2, x=x)
    assert np.array_equal(got.values, want.values)
    assert np.array_equal(np.array(fresh.fetch("st")), np.array(vgp_like.fetch("st")))
    r = got.problem(0)
    st = np.asarray(fresh.fetch("st")).reshape(9, 12, 12)
    assert np.array_equal(r.cov(0, 0), st[0]) and np.array_equal(r.cov(0, 2), r.cov(2, 0).T)
    assert np.array_equal(r.joint()[12:, 12:], st[2])
    assert np.allclose(np.diag(r.corr(2, 2)), 1.0, rtol=1e-15)
    assert np.all(np.linalg.eigvalsh((r.joint() + r.joint().T) / 2) > 0)
    fresh.close()
    vgp_like.close()
    # an ODE-only context and a context without a model know the propagator
    ode = va.Context("NONE", "rk4", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    xo = np.random.default_rng(1).standard_normal((2, 10 * 12))
    out = ode.lag_covariance([0, 9], "propagator", x=xo)
    assert out.values.shape == (2, 2, 10, 3, 3) and np.array_equal(out.values[:, 1, 9], np.broadcast_to(np.eye(3), (2, 3, 3)))
    with pytest.raises(RuntimeError):
        ode.lag_covariance([0], "covariance")
    ode.close()
    # VarGP and ProblemBatch: one record per problem, the member's own x
    ps = [build_problem("L96", "rk4", 0.5, dim_d=12, seed=SEED + j) for j in range(2)]
    pb = va.ProblemBatch([q["vgp"] for q in ps])
    xb = pb.initialization()
    recs = pb.posterior_kernel([0, 10], stride=5, x=xb)
    props = pb.posterior_kernel([0, 10], kind="propagator", stride=5)
    assert len(recs) == 2 and recs[0].values.shape == (2, 11, 12, 12) and list(recs[1].grid) == list(range(0, 51, 5))
    for j, q in enumerate(ps):
        one = q["vgp"].posterior_kernel([0, 10], kind="propagator", stride=5, x=xb[j])
        assert np.array_equal(one.values, props[j].values), j
        k = q["vgp"].posterior_kernel([0, 10], stride=5, x=xb[j])
        assert k.values.shape == (2, 11, 12, 12) and np.all(np.linalg.eigvalsh(k.joint()) > 0)
        assert np.allclose(k.values, recs[j].values, rtol=1e-12, atol=0.0)
        q["vgp"].close() if hasattr(q["vgp"], "close") else None
    pb.close()


def test_errors_and_limits():
    p, x = make_problem("L96", 12, 9)
    ctx = gpu_context(p)
    with pytest.raises(RuntimeError):
        ctx.lag_covariance([0], "covariance")                                # no cached state
    with pytest.raises(RuntimeError):
        ctx.lag_covariance([0], "propagator")                                # ... nor a cached x
    ctx.free_energy(x)
    want = ctx.lag_covariance([0, 3], "covariance", stride=2).values

    def same():
        assert np.array_equal(ctx.lag_covariance([0, 3], "covariance", stride=2).values, want)

    for bad in ([3, 0], [0, 0], [-1], [9], [0, 12], []):
        with pytest.raises(ValueError):
            ctx.lag_covariance(bad, "covariance")
        same()
    with pytest.raises(ValueError):
        ctx.lag_covariance([0], "covariance", stride=0)
    same()
    with pytest.raises(ValueError):
        ctx.lag_covariance([0], "cross")
    same()
    with pytest.raises(ValueError):
        ctx.lag_covariance([0.5], "covariance")
    # the C level: an unknown kind, null pointers, an x with the covariance kind
    lib, h = ctx._lib, ctx._h
    anchors = np.array([0, 3], dtype=np.int64)
    ap = anchors.ctypes.data_as(_lib.POINTER(_lib.c_int64))
    out = np.empty((1, 2, 9, 12, 12))
    xx = np.ascontiguousarray(x, dtype=np.float64)
    for args in ((7, None, 2, ap, 1, _lib._ptr(out)), (0, None, 2, ap, 1, None), (0, None, 2, None, 1, _lib._ptr(out)), (0, None, 0, ap, 1, _lib._ptr(out)),
                 (0, _lib._ptr(xx), 2, ap, 1, _lib._ptr(out))):
        rc = lib.vgpa_lag_covariance(h, *args)
        assert rc == -1, args
        with pytest.raises(ValueError):
            ctx._check(rc)
        same()
    assert lib.vgpa_lag_covariance(h, 0, None, 2, ap, 2, _lib._ptr(out)) == 0
    assert np.array_equal(out.ravel()[:want.size].reshape(want.shape), want)            # (stride 2: five kept rows, contiguous)
    ctx.close()
    # D > 64, resident and time-chunked: refused before any work, whatever the state
    p, x = make_problem("L96", 72, 5)
    for flags in (0, _lib.FLAG_STREAM_LARGE_D):
        big = gpu_context(p, flags=flags)
        with pytest.raises(NotImplementedError):
            big.lag_covariance([0], "propagator", x=x)
        f = big.free_energy(x)
        for kind in KINDS:
            with pytest.raises(NotImplementedError):
                big.lag_covariance([0], kind)
        assert abs(big.free_energy(x) - f) <= 1e-12 * abs(f)
        big.close()


def test_worst_ratios_of_the_module():
    """(runs last) the worst err_k / max(err_o, 2^-53) per kind of the rounding cases that ran in this process"""
    for kind, worst in sorted(WORST.items()):
        print(f"{kind}: worst err_k / max(err_o, 2^-53) = {worst:.2f}")
        assert worst <= 32.0
