"""
The two-time covariance of the posterior process, K(k, s) = Phi(k, s) S_s, and its propagator Phi(k, s) (vgpa_lag_covariance, DESIGN.md
s.4.19) -- what runs without a GPU: the C surface and the Python surface, the references the GPU file (test_lag_covariance.py) holds the
device against, the properties of the recursion itself, the GPU file's case table, and the result class on hand-made arrays.

References.  Every column of C_k = Phi(k, s) C_s obeys the MEAN recursion with b = 0, so the yardsticks exist already:
  lag_numpy   fp64: oracle.solve_fwd(...)[0] column by column with off_b = 0, started at the anchor
  lag_ld      np.longdouble: the same recursion on whole matrices, held against extended_ref.solve_fwd column by column below
Errors are relative in the max norm of one D x D block (one case, one anchor, one kept k); the device's err_k and the fp64 oracle's err_o are
both measured against lag_ld, and the project's bound is err_k <= 32 max(err_o, 2^-53).

Case table (CASES): models OU, double well (D = 1), Lorenz-63 (D = 3), Lorenz-96 at D = 5, 12, 17, 33, 40, 44, 63, 64 -- a ragged 4-block, a
ragged 16-tile, the 33 .. 40 cover's range, above 44, the edges of the last tile --, all four methods, Np in {2, 3, 9, 33}, the anchors {0},
{Np - 1}, {0, 1}, a middle one off the kept grid and every index, stride in {1, 2, 3}, both kinds (every case runs both), B in {1, 3} with
per-problem x, in two input regimes: benign (make_problem of test_gpu_edge_cases: A_t = 8 I + 0.05 noise, dt = 0.01) and stiff (the dense
A_t of test_stepper_rounding: dt rho(A_t) = 0.45, RK4 0.9).  The cross product is thinned by cycling the values with coprime periods;
test_case_table_meets_the_coverage_conditions says what the thinning keeps.  One adjustment for the references' cost (column by column through
the oracle): "every index" above D = 17 runs on at most 9 grid points.

The statistical case links the propagator to the sampler: for Euler-Maruyama Cov[x_k, x_s] = Phi(k, s) Var[x_s] exactly in expectation, so the
empirical cross-covariance of n = 4096 posterior paths must agree with Phi(k, s) Var_EM[x_s] to the Gaussian standard error of a sample
covariance, sqrt((V_ii(k) V_jj(s) + K_ij^2) / n), times 6 -- derived, not tuned.  Here the numpy sampler meets it for the committed seed;
the GPU file asks the same of the device's sampler and the device's Phi.
"""
import collections
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.lagcov import LagCovariance
from conftest import ROOT
from extended_ref import _ld, kappa
from extended_ref import solve_fwd as solve_fwd_ld
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import make_problem
from test_sample_paths_cpu import em_moments, sample_paths_numpy
from test_stepper_rounding_cpu import FACTOR, METHODS, UNIT, bound, stiff_ab

LD = np.longdouble
KINDS = ("covariance", "propagator")
ORDER = {"euler": 1, "heun": 2, "rk2": 2, "rk4": 4}


# --------------------------------------------------------------------------- #
#  The references
# --------------------------------------------------------------------------- #
def n_keep(n_pts, stride):
    return (n_pts - 1) // stride + 1


def _as_matrices(lin_a):
    """A_t as (n, D, D): the 1-D models' (n,) arrays are 1 x 1 matrices"""
    lin_a = np.asarray(lin_a)
    return lin_a.reshape(-1, 1, 1) if lin_a.ndim == 1 else lin_a


def lag_numpy(method, dt, lin_a, start, s, stride):
    """(n_keep, D, D) fp64: rows k >= s from oracle.solve_fwd's mean branch with off_b = 0, one column of `start` at a time, started at the
    anchor; rows before the anchor are zero.  1-D models ((n,) lin_a): the oracle's scalar branch."""
    single = np.ndim(lin_a) == 1
    a = np.asarray(lin_a, dtype=float)
    n = a.shape[0]
    d = 1 if single else a.shape[1]
    start = np.asarray(start, dtype=float).reshape(d, d)
    cols = np.zeros((n, d, d))
    if single:
        cols[s:, 0, 0] = vo.solve_fwd(method, dt, True, a[s:], np.zeros(n - s), start[0, 0], 0.0, 0.0)[0]
    else:
        zero = np.zeros((d, d))
        for j in range(d):
            cols[s:, :, j] = vo.solve_fwd(method, dt, False, a[s:], np.zeros((n - s, d)), start[:, j], zero, zero)[0]
    out = np.zeros((n_keep(n, stride), d, d))
    kept = np.arange(0, n, stride)
    out[kept >= s] = cols[kept[kept >= s]]
    return out


def lag_ld(method, dt, lin_a, start, s, stride):
    """(n_keep, D, D) np.longdouble: the recursion of extended_ref.solve_fwd's mean branch with b = 0 on all columns at once"""
    a = _ld(_as_matrices(lin_a))
    n, d = a.shape[0], a.shape[1]
    dt = LD(dt)
    h = dt / 2
    c = _ld(start).reshape(d, d).copy()
    out = np.zeros((n_keep(n, stride), d, d), dtype=LD)
    if s % stride == 0:
        out[s // stride] = c
    for k in range(s, n - 1):
        ak, ap = a[k], a[k + 1]
        am = (ak + ap) / 2
        if method == "euler":
            c = c + (-ak.dot(c)) * dt
        elif method == "heun":
            p = -ak.dot(c)
            c = c + h * (p + (-ap.dot(c + p * dt)))
        elif method == "rk2":
            c = c + dt * (-am.dot(c + h * (-ak.dot(c))))
        elif method == "rk4":
            k1 = -ak.dot(c)
            k2 = -am.dot(c + h * k1)
            k3 = -am.dot(c + h * k2)
            k4 = -ap.dot(c + dt * k3)
            c = c + dt * (k1 + 2 * (k2 + k3) + k4) / 6
        else:
            raise ValueError(f"unknown integration method: {method}")
        if (k + 1) % stride == 0:
            out[(k + 1) // stride] = c
    return out


def block_errors(got, ext, s, stride):
    """relative max-norm error of every kept block k >= s of got against ext (longdouble): {k: error}"""
    out = {}
    for j in range(ext.shape[0]):
        if j * stride >= s:
            out[j * stride] = float(np.max(np.abs(_ld(got[j]) - ext[j])) / np.max(np.abs(ext[j])))
    return out


# --------------------------------------------------------------------------- #
#  The GPU file's case table and inputs
# --------------------------------------------------------------------------- #
UNITS = [("OU", 1), ("DW", 1), ("L63", 3)] + [("L96", d) for d in (5, 12, 17, 33, 40, 44, 63, 64)]
N_PTS = (2, 3, 9, 33)
PATTERNS = ("first", "last", "first_two", "middle_off_grid", "every")
STRIDES = (1, 2, 3)
BATCHES = (1, 3)
REGIMES = ("benign", "stiff")
EVERY_MAX_D, EVERY_N_PTS = 17, 9          # "every index" above D = 17: at most 9 grid points (the cost of the column-by-column oracle)
Case = collections.namedtuple("Case", "model d method n_pts pattern stride batch regime")


def kernel_family(d):
    """which kernel of lag_cov.hip a D runs: the lane kernel, or the matrix-core kernel of tile NT = 16, 32, 48, 64"""
    return "lane" if d <= 4 else "mfma%d" % (16 * ((d + 15) // 16))


def _cases():
    """units x regimes x two method shifts; unit u runs method (u + r + shift) mod 4 in regime r -- every unit sees all four methods; D = 17,
    the one unit of its tile, runs all four shifts: every method in both regimes --, and Np, the anchors, the stride and the batch cycle with
    the running index (periods 4, 5, 3 and 2 on i + u, i, i and i // 3)"""
    cases, i = [], 0
    alone = {f for f in {kernel_family(d) for _, d in UNITS} if sum(kernel_family(d) == f for _, d in UNITS) == 1}
    for u, (model, d) in enumerate(UNITS):
        for r, regime in enumerate(REGIMES):
            for shift in ((0, 1, 2, 3) if kernel_family(d) in alone else (0, 2)):
                n_pts, pattern, stride, batch = N_PTS[(i + u) % 4], PATTERNS[i % 5], STRIDES[i % 3], BATCHES[(i // 3) % 2]
                if pattern == "middle_off_grid" and stride == 1:
                    stride = 2
                if pattern == "every" and d > EVERY_MAX_D:
                    n_pts = min(n_pts, EVERY_N_PTS)
                cases.append(Case(model, d, METHODS[(u + r + shift) % 4], n_pts, pattern, stride, batch, regime))
                i += 1
    return cases


CASES = _cases()


def case_id(c):
    return "-".join(str(v) for v in c)


def anchors_of(c):
    n = c.n_pts
    if c.pattern == "first":
        return [0]
    if c.pattern == "last":
        return [n - 1]
    if c.pattern == "first_two":
        return [0, 1]
    if c.pattern == "every":
        return list(range(n))
    s = n // 2
    if s % c.stride == 0:
        s += 1 if s + 1 < n else -1
    return [s]


@functools.lru_cache(maxsize=None)
def case_problem(c):
    return make_problem(c.model, c.d, c.n_pts, method=c.method)


@functools.lru_cache(maxsize=None)
def case_x(c, k):
    """x of problem k of the case (each problem has its own)"""
    p, x = case_problem(c)
    rng = np.random.default_rng([CASES.index(c), k, 19])
    if c.regime == "benign":
        return x + (0.05 if p.single_dim or c.model == "L63" else 0.02) * rng.standard_normal(x.size)
    a, b = stiff_ab(rng, c.d, c.n_pts, c.method)
    return np.concatenate((a.ravel(), b.ravel()))


def case_a(c, k):
    """A_t of problem k as the oracle takes it: (Np,) for the 1-D models, else (Np, D, D)"""
    p, _ = case_problem(c)
    a = case_x(c, k)[:c.n_pts * c.d * c.d]
    return a if p.single_dim else a.reshape(c.n_pts, c.d, c.d)


def case_start(c, k, s, kind, st=None):
    """C_s: the identity, or S_s -- of st (Np, D, D) when given (the GPU file passes what the device holds), else of the oracle's forward sweep"""
    if kind == "propagator":
        return np.eye(c.d)
    if st is None:
        p, _ = case_problem(c)
        lin_a, off_b = p.split(case_x(c, k))
        st = vo.solve_fwd(p.method, p.dt, p.single_dim, lin_a, off_b, p.m0, p.s0, p.sigma)[1]
    return np.asarray(st, dtype=float).reshape(c.n_pts, c.d, c.d)[s]


def case_reference(c, k, s, kind, st=None):
    """(lag_ld, lag_numpy) of problem k, anchor s"""
    p, _ = case_problem(c)
    start = case_start(c, k, s, kind, st)
    return lag_ld(c.method, p.dt, case_a(c, k), start, s, c.stride), lag_numpy(c.method, p.dt, case_a(c, k), start, s, c.stride)


def test_case_table_meets_the_coverage_conditions():
    assert {(c.model, c.d) for c in CASES} == set(UNITS)
    assert {d for m, d in UNITS if m == "L96"} == {5, 12, 17, 33, 40, 44, 63, 64}
    for name, values in (("n_pts", N_PTS), ("pattern", PATTERNS), ("stride", STRIDES), ("batch", BATCHES), ("regime", REGIMES), ("method", METHODS)):
        assert {getattr(c, name) for c in CASES} == set(values), name
    families = {kernel_family(d) for _, d in UNITS}
    assert families == {"lane", "mfma16", "mfma32", "mfma48", "mfma64"}
    # every kernel instantiation (family x method) in both regimes; every family on every grid length, anchor pattern, stride and batch
    assert {(kernel_family(c.d), c.method, c.regime) for c in CASES} == {(f, m, r) for f in families for m in METHODS for r in REGIMES}
    for name, values in (("n_pts", N_PTS), ("pattern", PATTERNS), ("stride", STRIDES), ("batch", BATCHES)):
        for f in families:
            assert {getattr(c, name) for c in CASES if kernel_family(c.d) == f} == set(values), (f, name)
    for c in CASES:
        a = anchors_of(c)
        assert a == sorted(set(a)) and 0 <= a[0] and a[-1] < c.n_pts, c
        if c.pattern == "middle_off_grid":
            assert c.stride >= 2 and a[0] % c.stride != 0, c
        if c.pattern == "every" and c.d > EVERY_MAX_D:
            assert c.n_pts <= EVERY_N_PTS
    assert any(c.pattern == "every" and c.n_pts == 33 for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_is_in_its_regime_and_the_oracle_error_is_finite(c):
    p, _ = case_problem(c)
    assert p.dt == 0.01
    a = _as_matrices(case_a(c, 0))
    rho = np.max(np.abs(np.linalg.eigvals(a)), axis=1)
    if c.regime == "stiff":
        np.testing.assert_allclose(p.dt * rho, 0.9 if c.method == "rk4" else 0.45, rtol=1e-10)
    else:
        assert np.all(p.dt * rho < 0.25)
    if c.batch > 1:
        assert not np.array_equal(case_x(c, 0), case_x(c, c.batch - 1))
    anchors = anchors_of(c)
    for s in sorted({anchors[0], anchors[-1]}):
        for kind in KINDS:
            ext, orc = case_reference(c, 0, s, kind)
            errs = block_errors(orc, ext, s, c.stride)
            assert len(errs) == sum(1 for k in range(0, c.n_pts, c.stride) if k >= s)
            assert all(np.isfinite(e) for e in errs.values()), (s, kind, errs)
            assert all(e <= 1e-11 for e in errs.values()), (s, kind, errs)          # (a restatement error is not a rounding error)
            assert np.isfinite(bound(max(errs.values(), default=0.0)))


# --------------------------------------------------------------------------- #
#  The C surface and the Python surface
# --------------------------------------------------------------------------- #
def test_symbol_prototype_and_enum():
    assert "vgpa_lag_covariance" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header)
    assert _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_lag_covariance\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, int kind, const double* x_or_null, int32_t n_anchor, const int64_t* anchors, int32_t stride, "
                    "double* out")
    assert re.search(r"enum\s*\{\s*VGPA_LAG_COVARIANCE\s*=\s*0\s*,\s*VGPA_LAG_PROPAGATOR\s*=\s*1\s*\}", header)
    assert _lib.LAG_KINDS == {"covariance": 0, "propagator": 1}
    with open(os.path.join(ROOT, "vgpa_amd", "build.py")) as fh:
        assert '"lag_cov.hip"' in fh.read()
    assert os.path.exists(os.path.join(ROOT, "vgpa_amd", "csrc", "lag_cov.hip"))


def test_python_surface():
    for owner, name, params in [(va.Context, "lag_covariance", ["anchors", "kind", "stride", "x"]),
                                (va.VarGP, "posterior_kernel", ["anchors", "kind", "stride", "x"]),
                                (va.ProblemBatch, "posterior_kernel", ["anchors", "kind", "stride", "x"])]:
        fn = getattr(owner, name, None)
        assert callable(fn), (owner.__name__, name)
        got = list(inspect.signature(fn).parameters)[1:]
        assert got == params, (owner.__name__, name, got)
        sig = inspect.signature(fn).parameters
        assert sig["kind"].default == "covariance" and sig["stride"].default == 1 and sig["x"].default is None
    for name in ("grid", "cov", "corr", "joint", "increment_var"):
        assert name in dir(LagCovariance) or name == "grid"
    assert list(LagCovariance(np.zeros((1, 3, 2, 2)), [0], [0, 2, 4]).grid) == [0, 2, 4]


def test_the_product_does_not_import_the_oracle():
    for name in ("lagcov.py", "_lib.py", "variational.py", "batch.py"):
        with open(os.path.join(ROOT, "vgpa_amd", name)) as fh:
            src = fh.read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), name


# --------------------------------------------------------------------------- #
#  The recursion itself
# --------------------------------------------------------------------------- #
def _benign_a(d, n, seed=3):
    rng = np.random.default_rng(seed)
    return 8.0 * np.eye(d) + 0.05 * rng.standard_normal((n, d, d))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("d", [1, 3, 5])
def test_longdouble_restatement_equals_extended_ref_column_by_column(method, d):
    n, s, dt = 7, 2, 0.01
    rng = np.random.default_rng([d, 11])
    a = _benign_a(d, n)
    start = rng.standard_normal((d, d))
    got = lag_ld(method, dt, a, start, s, 1)
    zero = np.zeros((d, d))
    for j in range(d):
        want = solve_fwd_ld(method, dt, a[s:], np.zeros((n - s, d)), start[:, j], zero, zero)[0]
        assert np.array_equal(got[s:, :, j], want), (method, d, j)
    # ... and the scalar models' 1-D arrays
    a1 = 1.6 + 0.05 * rng.standard_normal(n)
    got1 = lag_ld(method, dt, a1, 0.7, s, 1)
    assert np.array_equal(got1[s:, 0, 0], solve_fwd_ld(method, dt, a1[s:], np.zeros(n - s), 0.7, 0.0, 0.0)[0])
    err = block_errors(lag_numpy(method, dt, a1, 0.7, s, 1), got1, s, 1)
    assert max(err.values()) <= 64 * UNIT


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("stride", STRIDES)
def test_rows_before_the_anchor_are_zero_and_row_s_is_the_start(method, stride):
    d, n, dt = 4, 11, 0.01
    a = _benign_a(d, n)
    start = np.random.default_rng(5).standard_normal((d, d))
    for s in (0, 3, 4, 6, n - 1):
        for fn in (lag_numpy, lag_ld):
            out = fn(method, dt, a, start, s, stride)
            assert out.shape == (n_keep(n, stride), d, d)
            for j in range(out.shape[0]):
                if j * stride < s:
                    assert not np.any(out[j]), (s, j)
                elif j * stride == s:
                    assert np.array_equal(out[j], start), (s, j)      # exactly
                else:
                    assert np.any(out[j])
        # a kept row does not depend on the stride
        full = lag_numpy(method, dt, a, start, s, 1)
        assert np.array_equal(lag_numpy(method, dt, a, start, s, stride), full[::stride])


@pytest.mark.parametrize("method", METHODS)
def test_semigroup(method):
    """Phi(k, s) = Phi(k, r) Phi(r, s), entry by entry to 32 2^-53 kappa, kappa = sum |terms| / |sum| of that entry's inner product"""
    d, n, dt = 5, 9, 0.01
    a = _benign_a(d, n)
    eye = np.eye(d)
    for s, r in ((0, 4), (2, 3), (1, 7)):
        phi_s = lag_numpy(method, dt, a, eye, s, 1)
        phi_r = lag_numpy(method, dt, a, eye, r, 1)
        for k in range(r, n):
            terms = phi_r[k][:, :, None] * phi_s[r][None, :, :]            # [i, l, j]
            prod = _ld(terms).sum(axis=1)
            kap = kappa(terms, axis=1)
            err = np.abs(_ld(phi_s[k]) - prod) / np.abs(prod)
            assert np.all(err <= FACTOR * UNIT * kap), (method, s, r, k, float(np.max(err / kap)) / UNIT)


def test_euler_propagator_is_the_product_of_the_step_matrices():
    d, n, dt = 6, 9, 0.01
    a = _benign_a(d, n)
    phi = lag_ld("euler", dt, a, np.eye(d), 2, 1)
    t = _ld(np.eye(d))
    for k in range(2, n):
        assert float(np.max(np.abs(phi[k] - t)) / np.max(np.abs(t))) <= 4 * 2.0 ** -63 * (k - 1), k      # (longdouble: two roundings per step and entry)
        t = (_ld(np.eye(d)) - LD(dt) * _ld(a[k])).dot(t)
    got = lag_numpy("euler", dt, a, np.eye(d), 2, 1)
    assert max(block_errors(got, phi, 2, 1).values()) <= FACTOR * UNIT


@pytest.mark.parametrize("method", METHODS)
def test_ou_with_constant_a_converges_at_the_order_of_the_scheme(method):
    """K(t, s) -> exp(-a (t - s)) S_s: halving dt divides the error by 2^order"""
    a, s_s, span = 1.6, 0.37, 0.32
    errs = []
    for n in (9, 17):
        dt = span / (n - 1)
        got = lag_ld(method, dt, np.full(n, a), s_s, 0, 1)[-1, 0, 0]
        errs.append(abs(got - np.exp(LD(-a * span)) * LD(s_s)))
    order = float(np.log2(errs[0] / errs[1]))
    assert abs(order - ORDER[method]) < 0.15, (method, order)
    # an anchor in the middle sees the same law with its own S_s
    n, dt = 17, span / 16
    mid = lag_ld(method, dt, np.full(n, a), s_s, 8, 1)
    front = lag_ld(method, dt, np.full(n, a), s_s, 0, 1)
    assert np.allclose(np.asarray(mid[8:], dtype=float), np.asarray(front[:9], dtype=float), rtol=1e-15, atol=0.0)


# --------------------------------------------------------------------------- #
#  The link to the sampler
# --------------------------------------------------------------------------- #
STAT_SEED, STAT_PATHS, STAT_N_PTS, STAT_SIGMAS = 20261020, 4096, 33, 6.0
STAT_MODELS = (("L63", 3), ("L96", 12))
STAT_ANCHORS = (0, 10, 25)


def stat_problem(model, d):
    return make_problem(model, d, STAT_N_PTS, method="euler")


def check_sampler_link(paths, phi, var_em):
    """paths (n, Np, D); phi {s: (Np, D, D)} the propagator from anchor s; var_em (Np, D, D).  Every entry of the empirical Cov[x_k, x_s], k >= s,
    lies within STAT_SIGMAS standard errors of (Phi(k, s) Var_EM[x_s])_ij.  Returns the worst deviation in standard errors."""
    n = paths.shape[0]
    dev = paths - paths.mean(axis=0)
    worst = 0.0
    for s, phi_s in phi.items():
        for k in range(s, paths.shape[1]):
            emp = dev[:, k].T @ dev[:, s] / (n - 1)
            want = phi_s[k] @ var_em[s]
            se = np.sqrt((np.outer(np.diag(var_em[k]), np.diag(var_em[s])) + want ** 2) / n)
            z = np.abs(emp - want) / se
            worst = max(worst, float(z.max()))
            assert np.all(z <= STAT_SIGMAS), (s, k, float(z.max()))
    return worst


@pytest.mark.parametrize("model,d", STAT_MODELS)
def test_numpy_sampler_meets_the_statistical_bound(model, d):
    p, x = stat_problem(model, d)
    paths = sample_paths_numpy(p, "posterior", x, None, STAT_PATHS, 1, STAT_SEED)
    _, var_em = em_moments(p, x)
    a = x[:p.n_pts * d * d].reshape(p.n_pts, d, d)
    phi = {s: lag_numpy("euler", p.dt, a, np.eye(d), s, 1) for s in STAT_ANCHORS}
    worst = check_sampler_link(paths, phi, var_em)
    assert worst > 0.5        # (the check looked at something)
    # the identity behind it, without noise: Var_EM propagates as T S T^T + dt Sigma, so Cov_EM[x_k, x_s] = Phi(k, s) Var_EM[x_s] needs no more
    t = np.eye(d) - p.dt * a[0]
    assert np.allclose(phi[0][1], t, rtol=1e-15, atol=1e-18)


# --------------------------------------------------------------------------- #
#  The result class on hand-made arrays
# --------------------------------------------------------------------------- #
def _hand_made():
    """anchors 0 and 2 on a grid of 5 points kept with stride 1, D = 2: K(k, s) = F^(k - s) S_s, S_{k+1} = F S_k F^T + Q"""
    f = np.array([[0.9, 0.2], [-0.1, 0.8]])
    q = np.array([[0.05, 0.01], [0.01, 0.04]])
    st = [np.array([[1.0, 0.3], [0.3, 0.5]])]
    for _ in range(4):
        nxt = f @ st[-1] @ f.T + q
        st.append((nxt + nxt.T) / 2)                                 # symmetric to the bit
    st = np.array(st)
    anchors = [0, 2]
    values = np.zeros((2, 5, 2, 2))
    for i, s in enumerate(anchors):
        for k in range(s, 5):
            values[i, k] = np.linalg.matrix_power(f, k - s) @ st[s]
    return LagCovariance(values, anchors, np.arange(5)), st, f


def test_result_class_transpose_rule_and_key_errors():
    r, st, f = _hand_made()
    assert list(r.grid) == [0, 1, 2, 3, 4] and list(r.anchors) == [0, 2]
    assert np.array_equal(r.cov(3, 0), np.linalg.matrix_power(f, 3) @ st[0])
    assert np.array_equal(r.cov(0, 3), r.cov(3, 0).T)               # k < s: the transpose, from anchor k
    assert np.array_equal(r.cov(2, 4), r.cov(4, 2).T)
    assert np.array_equal(r.cov(2, 2), st[2]) and np.array_equal(r.cov(0, 0), st[0])
    for k, s in ((1, 3), (3, 1), (4, 3), (1, 1)):                    # neither index anchors the pair
        with pytest.raises(KeyError):
            r.cov(k, s)
    with pytest.raises(KeyError):
        r.cov(1, 2)                                                  # 1 < 2 and 1 is no anchor: K(2, 1) is not in the result
    strided = LagCovariance(np.zeros((1, 3, 2, 2)), [1], [0, 2, 4])
    with pytest.raises(KeyError):
        strided.cov(3, 1)                                            # 3 is not on the kept grid
    with pytest.raises(KeyError):
        strided.cov(1, 1)                                            # ... nor is the anchor itself
    with pytest.raises(ValueError):
        LagCovariance(np.zeros((2, 5, 2, 2)), [0, 2], np.arange(5), kind="propagator").cov(3, 0)
    with pytest.raises(ValueError):
        LagCovariance(np.zeros((2, 4, 2, 2)), [0, 2], np.arange(5))


def test_result_class_joint_corr_and_increment_var():
    r, st, f = _hand_made()
    j = r.joint()
    assert j.shape == (4, 4) and np.array_equal(j, j.T)
    assert np.array_equal(j[:2, :2], st[0]) and np.array_equal(j[2:, 2:], st[2])
    assert np.array_equal(j[2:, :2], r.cov(2, 0)) and np.array_equal(j[:2, 2:], r.cov(2, 0).T)
    assert np.all(np.linalg.eigvalsh(j) > 0)                         # a covariance
    want = st[2] + st[0] - r.cov(2, 0) - r.cov(2, 0).T
    assert np.array_equal(r.increment_var(2, 0), want)
    assert np.allclose(r.increment_var(0, 2), want, rtol=1e-15, atol=0.0)
    assert np.array_equal(r.increment_var(4, 2, st=st), st[4] + st[2] - r.cov(4, 2) - r.cov(4, 2).T)
    with pytest.raises(KeyError):
        r.increment_var(4, 2)                                        # without st, S_4 would have to be an anchor's first row
    c = r.corr(2, 0)
    assert np.allclose(c, r.cov(2, 0) / np.sqrt(np.outer(np.diag(st[2]), np.diag(st[0]))), rtol=1e-15, atol=0.0)
    assert np.allclose(np.diag(r.corr(0, 0)), 1.0, rtol=1e-15) and np.all(np.abs(c) <= 1.0)
    assert np.allclose(r.corr(4, 2, st=st), r.cov(4, 2) / np.sqrt(np.outer(np.diag(st[4]), np.diag(st[2]))), rtol=1e-15, atol=0.0)
    # a batch axis is carried through
    both = LagCovariance(np.stack([r.values, 2.0 * r.values]), r.anchors, r.grid)
    assert both.joint().shape == (2, 4, 4) and np.array_equal(both.problem(1).cov(3, 0), 2.0 * r.cov(3, 0))
    assert np.array_equal(both.cov(0, 3)[1], 2.0 * r.cov(3, 0).T)
