"""
The inputs, the case tables and the references of test_stepper_rounding.py (GPU), checked without a device, and the longdouble
restatement of the sweep (tests/extended_ref.py: solve_fwd, solve_bwd, obs_terms, the four energies, gradient, sweep) against the fp64
oracle.  The GPU module imports everything from here, so no GPU case rests on an input whose regime was not asserted.

The bound of both modules, per case and quantity q, in conftest.rel_err's norm evaluated in longdouble (xr-side: ld_rel_err):

    err_k(q) <= FACTOR * max(err_o(q), 2^-53)                                                  FACTOR = 32

err_o: the fp64 oracle against the restatement; err_k: what is tested (a kernel; here, a numpy mutant) against the restatement.

Three seeded regimes:
  * benign       -- the inputs of test_gpu_edge_cases.make_problem: A_t = 8 I + 0.05 noise, dt = 0.01 (h |A| = 0.08, near-diagonal);
  * stiff        -- A_t = c_t (1.5 I + G_t / sqrt(D)), G_t standard normal and different at every grid point, c_t such that
                    dt rho(A_t) = 0.45 (Euler, Heun, RK2) or 0.9 (RK4): dense, inside every method's stability region.  Operator level:
                    s0 = spd_with_spectrum(cond 1e6), a dense symmetric Sigma, b / slopes / jumps of size 10 ... 30, a jump at index 0
                    and one inside.  Fused level: the context's own Sigma and s0 with such A_t and b_t;
  * near-optimum -- fused level only: x* = 60 iterations of va.SCG on the oracle's free_energy / sweep (lean) from the benign x, where
                    the gradient is a small difference of large terms (asserted: max|gLb(x*)| <= max|gLb(x)| / 20).

Measured here, on the CPU (worst err_o over the compared problems of each table; every case prints its own):
  operator level  benign: m_t 3.6e-16, S_t 2.7e-16, lam_t 2.1e-16, Psi_t 2.1e-16;  stiff: m_t 2.8e-16, S_t 1.0e-15, lam_t 1.7e-16, Psi_t 5.2e-16
  fused, benign   F 1.7e-16, gLa 1.3e-15, gLb 1.3e-15, E_sde 6.8e-16, E_obs 3.4e-16, m_t 3.2e-16, S_t 2.8e-16, lam_t 1.0e-15, Psi_t 2.6e-15,
                  dEsde_dm 2.9e-15, dEsde_dS 6.4e-15 (cover kernels); the lane pass: dEsde_dS 1.6e-15, the rest below 1e-15
  fused, stiff    F 1.9e-16, gLa 2.8e-15, gLb 2.2e-15, lam_t 3.5e-15, dEsde_dm 4.9e-15 -- and dEsde_dS 9.7e-14 and, fed by it, Psi_t 1.4e-13
                  (cond(S_t) <= 4 there, so this is not the factorisation's conditioning; the bound follows err_o either way)
  fused, near     gLa 3.1e-14 (lane pass 5.3e-14), gLb 2.4e-13 (lane pass 3.0e-14), E_sde of the lane pass 2.5e-15 -- the cancellation, 20 ... 200 times the benign figure; everything else as benign
  so oracle and restatement agree to 2.4e-13 at worst, against RESTATEMENT_TOL = 1e-11.
The mutant (fourth RK4 slope of S_t and of Psi_t times 1 + 2^-30), D = 40: against the oracle S_t 1.1e-11 (benign) / 5.5e-11 (stiff), Psi_t
5.7e-11 / 8.9e-11 -- all pass 1e-9; err_k / max(err_o, 2^-53): S_t 7.1e4 / 1.8e5, Psi_t 3.5e5 / 5.2e5 -- three to four decimal orders over FACTOR.
The near-optimum drop of max|gLb|: 23x (D = 52) ... 118x (D = 37, N = 6) on the Lorenz-96 cases, 24x ... 105x on OU / double well / Lorenz-63.
"""
import collections
import functools

import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from conftest import rel_err
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import make_problem

LD = np.longdouble
FACTOR = 32
UNIT = 2.0 ** -53
METHODS = ("euler", "heun", "rk2", "rk4")
DT = 0.01
RESTATEMENT_TOL = 1e-11                    # oracle against restatement: a restatement error is not a rounding error (measured <= 1.5e-13)


def ld_rel_err(got, want):
    """conftest.rel_err's norm -- max|got - want| / max|want| -- evaluated in longdouble: the reference is not rounded to fp64 first."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def bound(err_o, extra=0.0):
    return FACTOR * max(err_o, UNIT) + extra


def ratio(err_k, err_o):
    return err_k / max(err_o, UNIT)


def checked(batch):
    """the problems of a batch that are compared: the first, the last, those next to 63 | 64"""
    return sorted({0, batch - 1} | ({63, 64} if batch > 64 else set()))


# --------------------------------------------------------------------------- #
#  Operator level: Context("NONE").solve_fwd / solve_bwd on arbitrary inputs
# --------------------------------------------------------------------------- #
# family, D, batch (CU_PLUS_1: one problem more than the device has compute units), flag name, VGPA_ODE_KERNEL, non-symmetric inputs, Np
CU_PLUS_1 = -1
Unit = collections.namedtuple("Unit", "family d batch flag env nonsym n_pts")
OP_UNITS = (
    [Unit("lane", 1, 3, None, None, True, 9), Unit("lane", 1, 520, None, None, True, 14)] +
    [Unit("lane", d, 520, None, None, True, 5 + 2 * d) for d in (2, 3, 4)] +
    [Unit("wave", d, 6, None, None, True, 2 + 3 * d) for d in (2, 3, 4)] +
    [Unit("pe", d, 2, None, None, False, n) for d, n in ((5, 14), (16, 7), (17, 10), (32, 6), (41, 9), (44, 5))] +
    [Unit("pe", 33, 2, None, "pe", False, 8), Unit("pe", 40, 2, None, "pe", False, 11)] +
    [Unit("sym", d, 2, None, None, False, n) for d, n in ((33, 7), (40, 12), (45, 6), (64, 5))] +
    [Unit("sym", 12, 2, "FLAG_SYM_UNITS", None, False, 13), Unit("sym", 36, CU_PLUS_1, None, None, False, 5)] +
    [Unit("generic", 7, 2, None, None, True, 10), Unit("generic", 40, 2, None, None, True, 6),
     Unit("generic", 12, 2, "FLAG_FORCE_GENERIC", None, False, 8)] +
    [Unit("large_d", 72, 1, None, None, False, 5), Unit("large_d", 130, 1, None, None, False, 5),
     Unit("large_d", 72, 1, "FLAG_STREAM_LARGE_D", None, False, 5)])
OP_REGIMES = ("benign", "stiff")
OpCase = collections.namedtuple("OpCase", Unit._fields + ("method", "regime"))


def _op_cases():
    """The cross product units x methods x regimes, thinned: unit i of a family runs method (i + r) mod 4 in regime r, and also
    (i + r + 2) mod 4 where the family has fewer than four units -- so every (family, method, regime) occurs and every unit runs in both
    regimes (test_operator_table_meets_the_coverage_conditions)."""
    cases = []
    for family in dict.fromkeys(u.family for u in OP_UNITS):
        units = [u for u in OP_UNITS if u.family == family]
        for i, u in enumerate(units):
            for r, regime in enumerate(OP_REGIMES):
                for shift in ((0,) if len(units) >= 4 else (0, 2)):
                    cases.append(OpCase(*u, METHODS[(i + r + shift) % 4], regime))
    return cases


OP_CASES = _op_cases()


def case_id(c):
    return "-".join(str(v) for v in c if v is not None and v is not False and v is not True)


def resolve_batch(c, n_cu=256):
    return n_cu + 1 if c.batch == CU_PLUS_1 else c.batch


def _sym(a):
    return (a + np.swapaxes(a, -1, -2)) / 2.0


def _sized(rng, shape):
    """entries of size 10 ... 30, either sign"""
    return rng.uniform(10.0, 30.0, shape) * rng.choice([-1.0, 1.0], shape)


def stiff_ab(rng, d, n_pts, method):
    """A_t = c_t (1.5 I + G_t / sqrt(D)) with dt rho(A_t) = 0.45 (RK4: 0.9) at every grid point, and b_t of size 10 ... 30."""
    target = 0.9 if method == "rk4" else 0.45
    a = 1.5 * np.eye(d) + rng.standard_normal((n_pts, d, d)) / np.sqrt(d)
    rho = np.max(np.abs(np.linalg.eigvals(a)), axis=1)
    return a * (target / (DT * rho))[:, None, None], _sized(rng, (n_pts, d))


@functools.lru_cache(maxsize=None)
def op_shared(c):
    """what every problem of the case shares: (m0, s0, Sigma)"""
    d = c.d
    rng = np.random.default_rng([c.d, c.n_pts, METHODS.index(c.method), OP_REGIMES.index(c.regime), 1])
    if c.regime == "benign":
        m0, s0, sigma = 8.0 + rng.standard_normal(d), 0.2 * np.eye(d), np.diag(3.0 + rng.random(d))
    else:
        q = rng.standard_normal((d, d)) / np.sqrt(d)
        m0, s0 = rng.standard_normal(d), xr.spd_with_spectrum(rng, d, 1e6, top=0.1)
        sigma = 4.0 * (np.eye(d) + 0.3 * _sym(q) + 0.3 * q.dot(q.T))
        sigma = _sym(sigma)
    if c.nonsym and d > 1:
        skew = rng.standard_normal((d, d))                  # (antisymmetric: the symmetric part keeps its spectrum)
        s0 = s0 + 0.01 * np.max(np.abs(s0)) * (skew - skew.T)
        sigma = sigma.copy()
        sigma[0, d - 1] += 0.1
    return m0, s0, sigma


@functools.lru_cache(maxsize=None)
def op_problem(c, k):
    """problem k of the case: (A, b, dEsde_dm, dEsde_dS, jump_m, jump_s) -- its own A_t; jumps at index 0 and inside"""
    d, n = c.d, c.n_pts
    rng = np.random.default_rng([c.d, c.n_pts, METHODS.index(c.method), OP_REGIMES.index(c.regime), 2, k])
    if c.regime == "benign":
        a = 8.0 * np.eye(d) + 0.05 * rng.standard_normal((n, d, d))
        b = 8.0 * op_shared(c)[0] + rng.standard_normal((n, d))
        draw = rng.standard_normal
    else:
        a, b = stiff_ab(rng, d, n, c.method)
        draw = functools.partial(_sized, rng)
    gm, gs = draw((n, d)), draw((n, d, d))
    jm, js = np.zeros((n, d)), np.zeros((n, d, d))
    for t in (0, n // 2):
        jm[t], js[t] = draw((d,)), draw((d, d))
    if not c.nonsym:
        gs, js = _sym(gs), _sym(js)
    return a, b, gm, gs, jm, js


OP_QUANTITIES = ("mt", "st", "lamt", "psit")


def _op_solve(fwd, bwd, c, k):
    m0, s0, sigma = op_shared(c)
    a, b, gm, gs, jm, js = op_problem(c, k)
    return dict(zip(OP_QUANTITIES, fwd(a, b, m0, s0, sigma) + bwd(a, gm, gs, jm, js)))


@functools.lru_cache(maxsize=None)
def op_reference(c, k):
    """(restatement, oracle) of problem k, each a dict over OP_QUANTITIES: once per session"""
    ext = _op_solve(functools.partial(xr.solve_fwd, c.method, DT), functools.partial(xr.solve_bwd, c.method, DT), c, k)
    orc = _op_solve(functools.partial(vo.solve_fwd, c.method, DT, False), functools.partial(vo.solve_bwd, c.method, DT, False), c, k)
    return ext, orc


def self_check(tag, ext, orc, worst):
    """oracle against restatement in every quantity: <= RESTATEMENT_TOL; err_o is printed (and kept in `worst`)"""
    for q in ext:
        err_o = ld_rel_err(orc[q], ext[q])
        print(f"{tag} {q}: err_o={err_o:.2e}")
        worst[q] = max(worst.get(q, 0.0), err_o)
        assert 0.0 <= err_o <= RESTATEMENT_TOL, (tag, q, err_o)
        assert np.all(np.isfinite(np.asarray(orc[q], dtype=float))), (tag, q)


WORST_OP = {}


@pytest.mark.parametrize("c", OP_CASES, ids=case_id)
def test_operator_case_is_in_its_regime_and_the_reference_holds(c):
    batch = resolve_batch(c)
    m0, s0, sigma = op_shared(c)
    assert (c.nonsym and c.d > 1) != (np.array_equal(s0, s0.T) and np.array_equal(sigma, sigma.T))
    for k in checked(batch):
        a, b, gm, gs, jm, js = op_problem(c, k)
        assert a.shape == (c.n_pts, c.d, c.d) and 5 <= c.n_pts <= 14
        assert np.any(jm[0]) and np.any(js[c.n_pts // 2]) and 0 < c.n_pts // 2 < c.n_pts - 1
        if not c.nonsym:                                   # (the matrix-core steppers are taken only on exactly symmetric arrays)
            assert np.array_equal(gs, np.swapaxes(gs, 1, 2)) and np.array_equal(js, np.swapaxes(js, 1, 2))
        rho = DT * np.max(np.abs(np.linalg.eigvals(a)), axis=1)
        ext, orc = op_reference(c, k)
        if c.regime == "stiff":
            assert np.all((0.4 <= rho) & (rho <= 1.0)), rho
            assert abs(np.linalg.cond(_sym(s0)) / 1e6 - 1.0) < 1e-3 or c.d == 1
            assert 10.0 <= np.min(np.abs(b)) and np.max(np.abs(gs)) <= 30.0
            with np.errstate(over="raise", invalid="raise", divide="raise"):      # no overflow
                vo.solve_fwd(c.method, DT, False, a, b, m0, s0, sigma), vo.solve_bwd(c.method, DT, False, a, gm, gs, jm, js)
            for s in orc["st"]:                            # positive definite, the smallest eigenvalue well above rounding
                lam = np.linalg.eigvalsh(_sym(s))
                assert lam[0] >= 1e-9 * lam[-1], (lam[0], lam[-1])
        else:
            assert np.all(rho < 0.1)
        self_check(f"[op {case_id(c)}] k={k}", ext, orc, WORST_OP.setdefault(c.regime, {}))


def test_operator_table_meets_the_coverage_conditions():
    """The thinned cross product keeps what it was thinned under (the table alone)."""
    families = {"lane", "wave", "pe", "sym", "generic", "large_d"}
    assert {(c.family, c.method, c.regime) for c in OP_CASES} == {(f, m, r) for f in families for m in METHODS for r in OP_REGIMES}
    for u in OP_UNITS:
        assert {c.regime for c in OP_CASES if c[:len(u)] == u} == set(OP_REGIMES), u
    def ds(family, **kw):
        return sorted(u.d for u in OP_UNITS if u.family == family and all(getattr(u, k) == v for k, v in kw.items()))
    assert ds("lane", batch=520) == [1, 2, 3, 4] and ds("lane", batch=3) == [1] and ds("wave", batch=6) == [2, 3, 4]
    assert ds("pe", env=None) == [5, 16, 17, 32, 41, 44] and ds("pe", env="pe") == [33, 40]
    assert ds("sym", flag=None, batch=2) == [33, 40, 45, 64] and ds("sym", flag="FLAG_SYM_UNITS") == [12] and ds("sym", batch=CU_PLUS_1) == [36]
    assert ds("generic", nonsym=True) == [7, 40] and ds("generic", flag="FLAG_FORCE_GENERIC") == [12]
    assert ds("large_d", flag=None) == [72, 130] and ds("large_d", flag="FLAG_STREAM_LARGE_D") == [72]
    assert all(u.n_pts == 5 for u in OP_UNITS if u.family == "large_d" or u.batch == CU_PLUS_1)
    assert len(OP_CASES) == len(set(OP_CASES))
    print("worst err_o, operator level:", {r: {q: f"{e:.1e}" for q, e in w.items()} for r, w in WORST_OP.items()})


# --------------------------------------------------------------------------- #
#  Fused level: Context.sweep / fetch / energy_parts against xr.sweep
# --------------------------------------------------------------------------- #
FusedCase = collections.namedtuple("FusedCase", "family model d n_pts method batch flag sigma regime")
FUSED_REGIMES = ("benign", "stiff", "near")
COVER_D = (33, 36, 37, 40)


def _cover_cases():
    """Every (D, method, batch side, regime) of the isotropic cover kernels; N rotates through {3, 6, 9} (near-optimum: {6, 9}, the same
    on both sides of 64 problems, which then share x*)."""
    cases = []
    for i, d in enumerate(COVER_D):
        for j, method in enumerate(("rk2", "rk4")):
            for s, batch in enumerate((3, 67)):
                for r, regime in enumerate(FUSED_REGIMES):
                    n = (6, 9)[(i + j) % 2] if regime == "near" else (3, 6, 9)[(i + j + s + r) % 3]
                    cases.append(FusedCase("cover", "L96", d, n, method, batch, None, "iso", regime))
    return cases


COVER_CASES = _cover_cases()
# one case each in the near-optimum and in the stiff regime: (family, D, Np, batch, flag name, Sigma form); "streamed" is the time-chunked
# sweep above D = 64, which only a fused context has (the flag changes nothing in an operator-level call)
PATHS = (("pe", 12, 9, 1, None, "diag"), ("sym_flag", 24, 9, 2, "FLAG_SYM_UNITS", "diag"), ("sym", 52, 9, 1, None, "diag"),
         ("keep_psi", 40, 6, 3, "FLAG_KEEP_PSI", "iso"), ("upper", 40, 9, 3, None, "diag"), ("generic", 12, 9, 2, "FLAG_FORCE_GENERIC", "diag"),
         ("large_d", 72, 9, 1, None, "diag"), ("streamed", 72, 9, 1, "FLAG_STREAM_LARGE_D", "diag"))
PATH_CASES = [FusedCase(f, "L96", d, n, METHODS[(i + r) % 4] if regime == "stiff" else "rk4", b, flag, sg, regime)
              for i, (f, d, n, b, flag, sg) in enumerate(PATHS) for r, regime in enumerate(("near", "stiff"))]
LANE_PASS_CASES = ([FusedCase("lane_pass", model, 1, 12, method, batch, None, "diag", regime)
                    for model in ("OU", "DW") for method in ("euler", "rk4") for batch in (1, 70) for regime in ("benign", "near")] +
                   [FusedCase("lane_pass", "L63", 3, 12, method, 520, None, "diag", regime) for method in METHODS for regime in ("benign", "near")])
FUSED_CASES = COVER_CASES + PATH_CASES + LANE_PASS_CASES
FUSED_QUANTITIES = ("F", "gLa", "gLb", "Esde", "Eobs", "mt", "st", "lamt", "psit", "dEsde_dm", "dEsde_ds")
NEAR_DROP = 20.0                              # max|gLb(x*)| <= max|gLb(x)| / NEAR_DROP
NEAR_SPREAD = 1e-7                            # the problems of a batch: x* (1 + NEAR_SPREAD noise) -- each its own x, all near the optimum


@functools.lru_cache(maxsize=None)
def fused_problem(model, d, n_pts, method, sigma):
    """the oracle problem and the benign x: two observations, at index 1 and at N - 2 (one at N = 3)"""
    return make_problem(model, d, n_pts, method=method, obs_at=sorted({1, n_pts - 2}), sigma=sigma)


def _sweep_fns(p):
    def f(x):
        return vo.free_energy(p, x, faithful=False)[0]

    def df(x, eval_fun=False):
        return vo.sweep(p, x, faithful=False)[1]
    return f, df


@functools.lru_cache(maxsize=None)
def near_optimum(model, d, n_pts, method, sigma):
    """x* = 60 iterations of va.SCG on the oracle's objective from the benign x: once per session"""
    p, x = fused_problem(model, d, n_pts, method, sigma)
    xs, _ = va.SCG(*_sweep_fns(p), {"max_it": 60, "x_tol": 0.0, "f_tol": 0.0})(x)
    return np.array(xs, dtype=float)


def glb_max(p, x):
    g = vo.sweep(p, x, faithful=False)[1]
    return float(np.max(np.abs(g[p.n_pts * p.dim_d ** 2:])))


@functools.lru_cache(maxsize=None)
def fused_x(c, k):
    """x of problem k of the case (each problem has its own)"""
    p, x = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    rng = np.random.default_rng([c.d, c.n_pts, METHODS.index(c.method), FUSED_REGIMES.index(c.regime), 3, k])
    if c.regime == "benign":
        return x + (0.05 if p.single_dim or c.model == "L63" else 0.02) * rng.standard_normal(x.size)
    if c.regime == "near":
        return near_optimum(c.model, c.d, c.n_pts, c.method, c.sigma) * (1.0 + NEAR_SPREAD * rng.standard_normal(x.size))
    a, b = stiff_ab(rng, c.d, c.n_pts, c.method)
    return np.concatenate((a.ravel(), b.ravel()))


def fused_quantities(p, f, g, state):
    k = p.n_pts * p.dim_d ** 2
    out = dict(F=f, gLa=g[:k], gLb=g[k:])
    out.update({q: state[q] for q in FUSED_QUANTITIES[3:]})
    return out


@functools.lru_cache(maxsize=None)
def fused_reference(c, k):
    """(restatement, oracle) of problem k, each a dict over FUSED_QUANTITIES: once per session"""
    p, _ = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    x = fused_x(c, k)
    f, gla, glb, state = xr.sweep(p, x, float(np.asarray(vo.kl0(p))))
    f_o, g_o, st_o = vo.sweep(p, x, faithful=False)
    return fused_quantities(p, f, np.concatenate((gla, glb)), state), fused_quantities(p, f_o, g_o, st_o)


WORST_FUSED = {}


@pytest.mark.parametrize("c", FUSED_CASES, ids=case_id)
def test_fused_case_is_in_its_regime_and_the_reference_holds(c):
    p, x0 = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    assert list(p.obs_t) == sorted({1, c.n_pts - 2})
    for k in checked(c.batch):
        x = fused_x(c, k)
        a, _ = p.split(x)
        if c.regime == "stiff":
            rho = DT * np.max(np.abs(np.linalg.eigvals(a)), axis=1)
            assert np.all((0.4 <= rho) & (rho <= 1.0)), rho
            with np.errstate(over="raise", invalid="raise", divide="raise"):      # the oracle raises nothing: no overflow, S_t positive definite throughout
                _, _, st = vo.sweep(p, x, faithful=False)
            for s in st["st"]:
                lam = np.linalg.eigvalsh(s)
                assert lam[0] >= 1e-9 * lam[-1], (lam[0], lam[-1])
        if c.regime == "near":
            before, after = glb_max(p, x0), glb_max(p, x)
            print(f"[fused {case_id(c)}] k={k}: max|gLb| {before:.3e} -> {after:.3e} ({before / after:.0f}x)")
            assert after <= before / NEAR_DROP
        ext, orc = fused_reference(c, k)
        self_check(f"[fused {case_id(c)}] k={k}", ext, orc, WORST_FUSED.setdefault((c.family, c.regime), {}))
    if c.batch > 1:                                        # every problem has its own x
        assert not np.array_equal(fused_x(c, 0), fused_x(c, c.batch - 1))


def test_fused_tables_meet_the_coverage_conditions():
    """The thinned tables keep what they were thinned under (the tables alone)."""
    assert {(c.d, c.method, c.batch >= 64, c.regime) for c in COVER_CASES} == \
        {(d, m, big, r) for d in COVER_D for m in ("rk2", "rk4") for big in (False, True) for r in FUSED_REGIMES}
    assert {c.batch for c in COVER_CASES} == {3, 67} and {c.n_pts for c in COVER_CASES} == {3, 6, 9}
    for r in FUSED_REGIMES:                                # every N on the separate assembly and on the gradient waves, in every regime it has
        want = {6, 9} if r == "near" else {3, 6, 9}
        assert {c.n_pts for c in COVER_CASES if c.regime == r and c.method == "rk4" and c.batch >= 64} == want, r
        assert {c.n_pts for c in COVER_CASES if c.regime == r and not (c.method == "rk4" and c.batch >= 64)} == want, r
    assert {(c.family, c.d, c.regime) for c in PATH_CASES} == {(f, d, r) for f, d, *_ in PATHS for r in ("near", "stiff")}
    assert [(f, d) for f, d, *_ in PATHS] == [("pe", 12), ("sym_flag", 24), ("sym", 52), ("keep_psi", 40), ("upper", 40), ("generic", 12), ("large_d", 72), ("streamed", 72)]
    assert {c.method for c in PATH_CASES if c.regime == "stiff"} == set(METHODS)
    lane = {(c.model, c.method, c.batch, c.regime) for c in LANE_PASS_CASES}
    assert lane == ({(m, s, b, r) for m in ("OU", "DW") for s in ("euler", "rk4") for b in (1, 70) for r in ("benign", "near")} |
                    {("L63", s, 520, r) for s in METHODS for r in ("benign", "near")})
    assert len(FUSED_CASES) == len(set(FUSED_CASES))
    print("worst err_o, fused level:", {k: {q: f"{e:.1e}" for q, e in w.items()} for k, w in WORST_FUSED.items()})


# --------------------------------------------------------------------------- #
#  The restatement additions on their own
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("model,d", [("OU", 1), ("DW", 1), ("L63", 3), ("L96", 12)])
@pytest.mark.parametrize("method", METHODS)
def test_restatement_equals_the_oracle_with_dense_noise_and_observation_operator(model, d, method):
    """xr.sweep against vo.sweep on make_problem(dense=True) with a non-identity H: dense Sigma, s0 and R (cholesky / tri_inverse /
    spd_inverse in obs_terms and gradient), observations whose counter differs from their index (Q4), every stepper.  The results are
    longdouble throughout (nothing was rounded on the way)."""
    rng = np.random.default_rng(11)
    single = d == 1
    h = None if single else np.eye(d) + 0.1 * rng.standard_normal((d, d))
    p, x = make_problem(model, d, 11, method=method, dense=not single, h_op=h, obs_at=[0, 4, 10])
    f, gla, glb, state = xr.sweep(p, x, float(np.asarray(vo.kl0(p))))
    f_o, g_o, st_o = vo.sweep(p, x, faithful=False)
    ext, orc = fused_quantities(p, f, np.concatenate((gla, glb)), state), fused_quantities(p, f_o, g_o, st_o)
    for q in ("Efx", "Edf", "dEobs_dm", "dEobs_ds"):
        ext[q], orc[q] = state[q], st_o[q]
    assert all(np.asarray(v).dtype == LD for v in ext.values())
    self_check(f"[restatement {model} {method}]", ext, orc, {})
    en = xr.model_energy(p, *p.split(x), state["mt"], state["st"])
    _, _, (_, _, dth, dsg) = vo.model_energy(p, *p.split(x), st_o["mt"], st_o["st"], faithful=False)
    assert ld_rel_err(dsg, en["dEsde_dsig"]) <= RESTATEMENT_TOL
    assert ld_rel_err(dth, en["dEsde_dth"]) <= RESTATEMENT_TOL


def test_scalar_recursions_take_the_oracles_one_dimensional_arrays():
    rng = np.random.default_rng(4)
    n = 9
    a, b, gm, gs = 1.6 + 0.3 * rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    jm, js = np.zeros(n), np.zeros(n)
    jm[[0, 5]], js[[0, 5]] = rng.standard_normal(2), rng.standard_normal(2)
    for method in METHODS:
        got = xr.solve_fwd(method, DT, a, b, 0.3, 0.2, 0.8) + xr.solve_bwd(method, DT, a, gm, gs, jm, js)
        want = vo.solve_fwd(method, DT, True, a, b, 0.3, 0.2, 0.8) + vo.solve_bwd(method, DT, True, a, gm, gs, jm, js)
        for g, w in zip(got, want):
            assert g.shape == (n,) and g.dtype == LD and ld_rel_err(w, g) <= 1e-15


# --------------------------------------------------------------------------- #
#  The bound closes the gap: a mutant that the 1e-9 of the older tests lets through
# --------------------------------------------------------------------------- #
def _mutant_rk4(c, k, eps=2.0 ** -30):
    """The oracle's RK4 (solve_fwd / solve_bwd, n-D) with the fourth slope of S_t forward and of Psi_t backward times 1 + eps."""
    m0, s0, sigma = op_shared(c)
    a, b, gm, gs, jm, js = op_problem(c, k)
    n, h = c.n_pts, 0.5 * DT
    mt, st = vo.solve_fwd("rk4", DT, False, a, b, m0, s0, sigma)
    st = st.copy()
    a_mid = 0.5 * (a[:-1] + a[1:])
    for i in range(n - 1):
        l1 = vo.f_s(st[i], a[i], sigma, False)
        l2 = vo.f_s(st[i] + h * l1, a_mid[i], sigma, False)
        l3 = vo.f_s(st[i] + h * l2, a_mid[i], sigma, False)
        l4 = vo.f_s(st[i] + DT * l3, a[i + 1], sigma, False) * (1.0 + eps)
        st[i + 1] = st[i] + DT * (l1 + 2.0 * (l2 + l3) + l4) / 6.0
    lam, _ = vo.solve_bwd("rk4", DT, False, a, gm, gs, jm, js)
    psi = np.zeros((n, c.d, c.d))
    am, es = vo._mid_padded(a), vo._mid_padded(gs)
    for t in range(n - 1, 0, -1):
        l1 = vo.f_psi(gs[t], a[t], psi[t], False)
        l2 = vo.f_psi(es[t - 1], am[t - 1], psi[t] - h * l1, False)
        l3 = vo.f_psi(es[t - 1], am[t - 1], psi[t] - h * l2, False)
        l4 = vo.f_psi(gs[t - 1], a[t - 1], psi[t] - DT * l3, False) * (1.0 + eps)
        psi[t - 1] = psi[t] - DT * (l1 + 2.0 * (l2 + l3) + l4) / 6.0 + js[t - 1]
    return dict(mt=mt, st=st, lamt=lam, psit=psi)


@pytest.mark.parametrize("regime", OP_REGIMES)
def test_a_slope_scaled_by_one_plus_2_to_the_minus_30_is_caught(regime):
    """D = 40, RK4: the mutant passes the suite's older check (rel_err < 1e-9 against the oracle) and misses the bound of this module
    in S_t and in Psi_t, in both regimes; with eps = 0 the same code IS the oracle (so the miss is the mutation's)."""
    c = OpCase("sym", 40, 2, None, None, False, 12, "rk4", regime)
    ext, orc = op_reference(c, 0)
    same = _mutant_rk4(c, 0, eps=0.0)
    assert all(np.array_equal(same[q], orc[q]) for q in OP_QUANTITIES)
    got = _mutant_rk4(c, 0)
    for q in OP_QUANTITIES:
        old, err_o, err_k = rel_err(got[q], orc[q]), ld_rel_err(orc[q], ext[q]), ld_rel_err(got[q], ext[q])
        print(f"[mutant {regime}] {q}: against the oracle {old:.2e}; err_o={err_o:.2e} err_k={err_k:.2e} ratio={ratio(err_k, err_o):.3g}")
        assert old < 1e-9
        assert (err_k <= bound(err_o)) == (q in ("mt", "lamt")), q
