"""
The inputs, the case tables and the references of test_obs_energy_rounding.py (GPU), checked without a device: the observation terms
(E_obs and both jumps), the closed-form energies of OU / double well / Lorenz-63 at operator level, dF/dtheta, and the fused paths of
the small models other than the lane pass -- each against the longdouble restatement of tests/extended_ref.py, with the fp64 oracle's
own error against it as the yardstick.  The GPU module imports everything from here, so no GPU case rests on an input whose regime was
not asserted.

The bound is test_stepper_rounding_cpu's, unchanged (FACTOR, UNIT, bound, ratio, ld_rel_err, checked, RESTATEMENT_TOL are imported):

    err_k(q) <= FACTOR * max(err_o(q), 2^-53)

One derived term, for the scalar results that are sums of terms of either sign -- E_obs, every component of dEsde_dth and of dF/dtheta:
a single number gets no averaging over entries, so the oracle may hit it by luck; its floor is kappa 2^-53 instead of 2^-53,
kappa = sum |summand| / |sum summand| over the summands of the restatement (xr.kappa): the per-observation terms and the normalisation
constant for E_obs, the trapezoid-weighted integrand values for the theta derivatives.  kappa = 1 where all summands have one sign, and
nothing changes there.  kbound / kratio below are bound / ratio with that floor.

Inputs (seeded; every regime is asserted by the test of its table):
  energies    benign: (A_t, b_t) of make_problem with the oracle's own (m_t, S_t); every-moment: |m|, S, A, b, theta of order one (Lorenz-63:
              S_t = d C d with correlations 0.8 / -0.6 / -0.5 and a dense non-symmetric A_t of size 5; double well: |m| ~ 1.5, s ~ 0.8)
              -- both fourth-moment cross terms of Lorenz-63 and every monomial of the double well's sixth moment carry >= 1e-2 of their
              moment at every grid point; residual-cancels: b_t such that <f> + A m - b ~ 1e-3 with S ~ 1e-3, dEsde_dm a small
              difference of large terms.
  observations  R diagonal with distinct entries / dense with cond 1e4 / I / (2 pi) (no normalisation constant: E_obs is the data-fit sum
              and the variance term alone), H None / an explicit identity / I + 0.1 noise / the mask diag(1, 0, 1, ...) / for the 1-D models the number h = 1.3, |y - m| of
              1, 1e-2, 1e-4 times |y|, observation indices that differ from their counter (Q4: asserted to move E_obs by more than the bound).

  dF/dtheta   the three energy regimes behind a fused evaluation (m0, s0 of the regime, b_t = A_t m0 + ... holding the mean there), and per
              model a case whose integrand changes sign along the grid (kappa above 1).
  fused       test_stepper_rounding_cpu's benign and near-optimum x on Lorenz-63 with 16 lanes per problem, VGPA_FLAG_MATERIALIZE and
              VGPA_FLAG_FORCE_GENERIC; every one of these paths again with three observations under a dense R / non-identity H (1-D: r = 0.07,
              h = 1.3), and such models per problem with ragged counts.

Measured here, on the CPU (worst err_o per table; every case prints its own):
  energies      benign 1.8e-15 (dEsde_dm); every-moment 1.6e-15 (dEsde_dth; the arrays <= 7.0e-16); residual-cancels: dEsde_dm 8.3e-13 (OU),
                2.2e-13 (double well), 1.6e-12 (Lorenz-63), dEsde_dth 1.3e-12, E_sde 4.8e-14 -- against RESTATEMENT_TOL = 1e-11
  observations  E_obs, vector jump and matrix jump each 1.9e-13 (dense R, cond 1e4: the factorisation; 2.8e-13 with a model per problem);
                diagonal R: <= 2.6e-16; S[t_n] for S[n] moves E_obs by at least 2.0e-5 of itself (bound of that case: 3.6e-15)
  dF/dtheta     6.7e-14 (residual-cancels); fused small paths: F, gradient, E_obs, lam_t and Psi_t 3.1e-13 (dense R), everything else <= 4.3e-15
  kappa         E_obs <= 1.71 (its normalisation constant is negative where |R| < 1); dEsde_dth <= 46.9 and dF/dtheta <= 19.5 (both on the
                residual-cancels inputs of Lorenz-63; the sign-changing cases: 1.2 ... 9.5)
  data-fit share of E_obs without its constant, |y - m| = 1, 1e-2, 1e-4 |y|: 0.82, 4.3e-4, 4.7e-8 (1-D, M = 257); 0.99, 8.0e-3, 8.0e-7 (D = 3)
  mutants       old check (1e-9 against the oracle on the golden / make_problem inputs) -> ratio err_k / max(err_o, kappa 2^-53) on the new inputs:
                2 Sxy^2 -> Sxy^2 in Lorenz-63's E[x^2 y^2]: 9.2e-12, passes -> 6.9e12;  15 s^3 (1 + 2^-30) in the double well's sixth
                moment: 4.9e-10, passes -> 7.5e5;  S[t_n] for S[n] in E_obs: 4.3e-4 and 6.7e-3, caught -> 4.0e10;  H^T R^-1 H for
                H^T R^-1 H^T in the vector jump: 0.16 where H is not symmetric, caught, and exactly 0 where H = I (the golden fixture),
                invisible -> 8.1e11
"""
import collections
import dataclasses
import functools

import numpy as np
import pytest

import extended_ref as xr
from conftest import load_golden, rel_err
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import make_problem, spd
from test_stepper_rounding_cpu import (FACTOR, FUSED_QUANTITIES, NEAR_DROP, RESTATEMENT_TOL, UNIT, FusedCase, bound, case_id, checked, fused_problem,
                                       fused_quantities, fused_reference, fused_x, glb_max, ld_rel_err, ratio)

LD = np.longdouble
DT = 0.01
SCALAR_SUMS = ("Eobs", "dEsde_dth", "dFdth")          # the quantities whose floor is kappa 2^-53: compared component by component


def kbound(err_o, kap=1.0):
    return FACTOR * max(err_o, kap * UNIT)


def kratio(err_k, err_o, kap=1.0):
    return err_k / max(err_o, kap * UNIT)


def pieces(q, value):
    """what is compared of quantity q: the array as a whole, or each component of a scalar sum on its own"""
    if q in SCALAR_SUMS:
        flat = np.atleast_1d(np.asarray(value)).ravel()
        return [(f"{q}[{i}]" if flat.size > 1 else q, flat[i]) for i in range(flat.size)]
    return [(q, value)]


def compare(tag, got, ext, orc, kappas, worst, passes=None, extra=None):
    """One line per call: for every piece  name err_o/err_k/ratio[/kappa]  (ratio = err_k / max(err_o, kappa 2^-53)).  Returns the pieces
    over their bound; `passes` counts the comparisons and those that only the kappa term let pass.  extra: quantity -> a derived term its
    bound gains (test_stepper_rounding.psi_recovery_term, for Psi_t where the plan has store_q; `+term` behind the ratio)."""
    fails, line = [], []
    for q in got:
        kap_q = np.atleast_1d(kappas.get(q, 1.0)).ravel()
        for i, ((name, g), (_, e), (_, o)) in enumerate(zip(pieces(q, got[q]), pieces(q, ext[q]), pieces(q, orc[q]))):
            kap = float(kap_q[i]) if q in SCALAR_SUMS else 1.0
            err_o, err_k = ld_rel_err(o, e), ld_rel_err(np.reshape(g, np.shape(e)), e)
            rat, more = kratio(err_k, err_o, kap), (extra or {}).get(q, 0.0)
            line.append(f"{name} {err_o:.1e}/{err_k:.1e}/{rat:.2f}" + (f"/k={kap:.3g}" if q in SCALAR_SUMS else "") + (f"+{more:.1e}" if more else ""))
            worst[q] = max(worst.get(q, 0.0), rat)
            if passes is not None:
                passes["n"] = passes.get("n", 0) + 1
                passes["kappa"] = passes.get("kappa", 0) + (bound(err_o) < err_k <= kbound(err_o, kap))
                passes["worst_kappa"] = max(passes.get("worst_kappa", 1.0), kap)
            if not err_k <= kbound(err_o, kap) + more:
                fails.append((tag, name, err_o, err_k, kbound(err_o, kap) + more))
    print(tag, " ".join(line))
    return fails


def self_check(tag, ext, orc, kappas, worst):
    """oracle against restatement in every piece: <= RESTATEMENT_TOL; err_o (and kappa) printed, the worst kept"""
    for q in ext:
        kap_q = np.atleast_1d(kappas.get(q, 1.0)).ravel()
        for i, ((name, e), (_, o)) in enumerate(zip(pieces(q, ext[q]), pieces(q, orc[q]))):
            err_o = ld_rel_err(o, e)
            print(f"{tag} {name}: err_o={err_o:.2e}" + (f" kappa={kap_q[i]:.3g}" if q in SCALAR_SUMS else ""))
            worst[q] = max(worst.get(q, 0.0), err_o)
            assert np.asarray(e).dtype == LD, (tag, name)
            assert 0.0 <= err_o <= RESTATEMENT_TOL, (tag, name, err_o)
            assert np.all(np.isfinite(np.asarray(o, dtype=float))), (tag, name)
            if q in SCALAR_SUMS:
                assert 1.0 <= kap_q[i] < 1e6, (tag, name, kap_q[i])


def _signed(rng, lo, hi, shape):
    return rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)


def _sym(a):
    return (a + np.swapaxes(a, -1, -2)) / 2.0


MODELS = ("OU", "DW", "L63")
MODEL_D = {"OU": 1, "DW": 1, "L63": 3}

# --------------------------------------------------------------------------- #
#  Energies, operator level: Context(model).energy(a, b, m, s, want_hyper=...)
# --------------------------------------------------------------------------- #
EnergyCase = collections.namedtuple("EnergyCase", "model regime n_pts batch hyper own")
E_REGIMES = ("benign", "moments", "residual")
E_NPTS = {"OU": (2, 255, 256, 257), "DW": (2, 255, 256, 257), "L63": (2, 63, 64, 65)}      # across the 256 (1-D) / 64 (L63) threads of a block
L63_CORR = np.array([[1.0, 0.8, -0.6], [0.8, 1.0, -0.5], [-0.6, -0.5, 1.0]])
E_QUANTITIES = ("Esde", "Ef", "Edf", "dEsde_dm", "dEsde_dS")
E_HYPER = ("dEsde_dth", "dEsde_dsig")


def _energy_cases():
    """Every (model, Np, regime); batch and want_hyper alternate so that every (model, regime) has both values of each, and all four
    (batch, want_hyper) pairs occur per model.  Last per model: per-problem theta / sigma rows (set_problem_params), three problems."""
    cases = []
    for model in MODELS:
        for i, n in enumerate(E_NPTS[model]):
            for r, regime in enumerate(E_REGIMES):
                cases.append(EnergyCase(model, regime, n, (1, 3)[((i >> 1) + r) % 2], bool((i + r) % 2), False))
        cases.append(EnergyCase(model, "moments", E_NPTS[model][-1], 3, True, True))
    return cases


ENERGY_CASES = _energy_cases()


def _mean_drift(model, theta, m, s):
    """<f> of the model in fp64 (the oracle's Ef expressions): what b_t is built from in the residual-cancels regime"""
    if model == "OU":
        return -theta * m
    if model == "DW":
        return 4.0 * (theta * m - (m ** 3 + 3 * m * s))
    v_s, v_r, v_b = theta
    return np.stack([v_s * (m[:, 1] - m[:, 0]), v_r * m[:, 0] - m[:, 1] - s[:, 2, 0] - m[:, 0] * m[:, 2],
                     s[:, 1, 0] + m[:, 0] * m[:, 1] - v_b * m[:, 2]], axis=1)


@functools.lru_cache(maxsize=None)
def energy_inputs(c, k):
    """problem k of the case: (theta, sigma, a, b, m, s); theta and sigma are shared by the batch unless c.own"""
    single, n = c.model in ("OU", "DW"), c.n_pts
    rng = np.random.default_rng([MODELS.index(c.model), E_REGIMES.index(c.regime), n, 7, k])
    if c.regime == "benign":
        p, x = make_problem(c.model, MODEL_D[c.model], n, obs_at=[1])
        a, b = p.split(x + 0.05 * rng.standard_normal(x.size))
        m, s = vo.solve_fwd("rk4", DT, single, a, b, p.m0, p.s0, p.sigma)
        theta, sigma, s = p.theta, p.sigma, (s if single else _sym(s))
    else:
        small = 1e-3 if c.regime == "residual" else 1.0
        if single:
            theta, sigma = (1.3 if c.model == "OU" else 1.0), 0.8
            a, m = _signed(rng, 0.5, 2.0, n), (_signed(rng, 0.5, 1.5, n) if c.model == "OU" else _signed(rng, 1.2, 1.8, n))
            s = small * (rng.uniform(0.5, 1.2, n) if c.model == "OU" else rng.uniform(0.6, 1.0, n))
            am = a * m
        else:
            theta, sigma = np.array([1.3, 0.9, 1.1]), np.diag([0.8, 1.0, 1.2])
            a, m = 5.0 * rng.standard_normal((n, 3, 3)), _signed(rng, 0.5, 1.0, (n, 3))
            dv = rng.uniform(0.9, 1.1, (n, 3))
            s = small * _sym(dv[:, :, None] * L63_CORR * dv[:, None, :])
            am = np.einsum("tij,tj->ti", a, m)
        if c.regime == "residual":
            b = _mean_drift(c.model, theta, m, s) + am - 1e-3 * _signed(rng, 0.5, 1.5, m.shape)
        else:
            b = _signed(rng, 0.5, 1.5, m.shape)
    if c.own:
        theta, sigma = theta * (1.0 + 0.1 * (k + 1)), sigma * (1.0 + 0.05 * (k + 1))
    return theta, sigma, a, b, m, s


def _energy_dicts(c, theta, sigma, a, b, m, s):
    names = E_QUANTITIES + (E_HYPER if c.hyper else ())
    fn = {"OU": xr.energy_ou, "DW": xr.energy_dw, "L63": xr.energy_l63}[c.model]
    ext = fn(theta, sigma, DT, a, b, m, s)
    if c.model == "L63":
        esde, (ef, edf), (dm, ds, dth, dsg) = vo.energy_l63(theta, vo.chol_inv(sigma)[0], DT, a, b, m, s, [])
    else:
        esde, (ef, edf), (dm, ds, dth, dsg) = (vo.energy_ou if c.model == "OU" else vo.energy_dw)(theta, sigma, DT, a, b, m, s, [])
    orc = dict(Esde=esde, Ef=ef, Edf=edf, dEsde_dm=dm, dEsde_dS=ds, dEsde_dth=dth, dEsde_dsig=dsg)
    kappas = {"dEsde_dth": xr.kappa(xr.trapezoid_summands(ext["dth_t"], DT), axis=0)}
    return {q: ext[q] for q in names}, {q: orc[q] for q in names}, kappas


@functools.lru_cache(maxsize=None)
def energy_reference(c, k):
    """(restatement, oracle, kappas) of problem k, the first two dicts over the case's quantities: once per session"""
    return _energy_dicts(c, *energy_inputs(c, k))


WORST_ENERGY = {}


@pytest.mark.parametrize("c", ENERGY_CASES, ids=case_id)
def test_energy_case_is_in_its_regime_and_the_reference_holds(c):
    for k in range(c.batch):
        theta, sigma, a, b, m, s = energy_inputs(c, k)
        m_l, s_l = np.asarray(m, dtype=LD), np.asarray(s, dtype=LD)
        if c.model == "L63":
            assert np.array_equal(s, np.swapaxes(s, 1, 2))
            for st in s:                                      # positive definite, well conditioned: no input leaves S_t indefinite
                lam = np.linalg.eigvalsh(st)
                assert lam[0] > 0 and lam[-1] / lam[0] <= 100.0, lam
        else:
            assert np.all(s > 0)
        if c.regime in ("moments", "residual") and c.model == "L63":
            assert 2.0 <= np.max(np.abs(a)) and not np.array_equal(a, np.swapaxes(a, 1, 2))
            corr = s / np.sqrt(np.einsum("tii->ti", s)[:, :, None] * np.einsum("tii->ti", s)[:, None, :])
            assert np.allclose(corr, L63_CORR, atol=1e-12)
        if c.regime == "moments":
            if c.model == "DW":                               # no monomial of the sixth moment is negligible
                mono = np.stack([m_l ** 6, 15 * m_l ** 4 * s_l, 45 * m_l ** 2 * s_l ** 2, 15 * s_l ** 3])
                share = float(np.min(mono / np.sum(mono, axis=0)))
                print(f"[energy {case_id(c)}] k={k}: smallest share of a monomial in ex6 {share:.3f}")
                assert share >= 1e-2
            if c.model == "L63":                              # both fourth-moment cross terms carry weight at every grid point
                for (i, j) in ((0, 1), (0, 2)):
                    mi, mj, sii, sjj, sij = m_l[:, i], m_l[:, j], s_l[:, i, i], s_l[:, j, j], s_l[:, i, j]
                    e4 = sii * (mj ** 2 + sjj) + sjj * mi ** 2 + 4 * sij * mi * mj + (mi * mj) ** 2 + 2 * sij ** 2
                    share = float(np.min(2 * sij ** 2 / e4))
                    print(f"[energy {case_id(c)}] k={k}: smallest share of 2 S{i}{j}^2 in its fourth moment {share:.3f}")
                    assert share >= 1e-2
        if c.regime == "residual":
            am = a * m if c.model != "L63" else np.einsum("tij,tj->ti", a, m)
            resid = np.abs(_mean_drift(c.model, theta, m, s) + am - b)
            assert np.all((3e-4 <= resid) & (resid <= 2e-3)), (resid.min(), resid.max())
            assert np.max(np.abs(s)) <= 1.5e-3
        ext, orc, kappas = energy_reference(c, k)
        self_check(f"[energy {case_id(c)}] k={k}", ext, orc, kappas if c.hyper else {}, WORST_ENERGY.setdefault(c.regime, {}))
    if c.own:
        assert not np.array_equal(energy_inputs(c, 0)[0], energy_inputs(c, c.batch - 1)[0])


def test_energy_table_meets_the_coverage_conditions():
    shared = [c for c in ENERGY_CASES if not c.own]
    assert {(c.model, c.n_pts, c.regime) for c in shared} == {(m, n, r) for m in MODELS for n in E_NPTS[m] for r in E_REGIMES}
    for m in MODELS:
        for r in E_REGIMES:
            assert {c.hyper for c in shared if (c.model, c.regime) == (m, r)} == {False, True}
            assert {c.batch for c in shared if (c.model, c.regime) == (m, r)} == {1, 3}
        assert {(c.batch, c.hyper) for c in shared if c.model == m} == {(b, h) for b in (1, 3) for h in (False, True)}
        assert [c for c in ENERGY_CASES if c.own and c.model == m] == [EnergyCase(m, "moments", E_NPTS[m][-1], 3, True, True)]
    assert all(n <= 258 for n in E_NPTS["OU"]) and all(n <= 65 for n in E_NPTS["L63"])
    assert len(ENERGY_CASES) == len(set(ENERGY_CASES))
    print("worst err_o, energies:", {r: {q: f"{e:.1e}" for q, e in w.items()} for r, w in WORST_ENERGY.items()})


# --------------------------------------------------------------------------- #
#  Observation terms, operator level: Context.obs_energy(m, s)
# --------------------------------------------------------------------------- #
ObsCase = collections.namedtuple("ObsCase", "d m_obs n_pts r_form h_form scale")
R_FORMS, H_FORMS = ("diag", "dense", "nonorm"), (None, "eye", "noise", "mask", "scalar")
SCALAR_H = 1.3                                    # the observation operator of a 1-D model is a number: the vector jump is -(y - h m) / r
O_SCALES = (1.0, 1e-2, 1e-4)
ND_SHAPES = ((3, 1, 2), (3, 85, 86), (3, 86, 87), (12, 22, 30), (64, 5, 9))      # D M across 256 at D = 3; (D, M, Np)
LARGE_SHAPES = tuple((d, m, 5) for d in (72, 257) for m in (1, 3))
ALL_FORMS = (("diag", None), ("diag", "eye"), ("diag", "noise"), ("diag", "mask"), ("dense", None), ("dense", "noise"), ("dense", "mask"))
OBS_CASES = ([ObsCase(1, m, m + 1, "diag", None, 0.1) for m in (1, 256, 257)] + [ObsCase(1, 257, 258, "diag", "scalar", 0.1)] +
             [ObsCase(1, 257, 258, "nonorm", None, sc) for sc in O_SCALES] +
             [ObsCase(d, m, n, r, h, 0.1) for d, m, n in ND_SHAPES for r, h in (ALL_FORMS if (d, m) == (3, 86) else ALL_FORMS[:2] + ALL_FORMS[5:6])] +
             [ObsCase(3, 85, 86, "nonorm", None, sc) for sc in O_SCALES] +
             [ObsCase(d, m, n, r, h, 0.1) for d, m, n in LARGE_SHAPES for r, h in (("diag", None), ("dense", "noise"))])
O_QUANTITIES = ("Eobs", "jm", "js")


def takes_diag_branch(c):
    """obs_constants: diagonal R and H = I (None or an explicit identity) -> a.diag; 1-D has one form"""
    return c.r_form in ("diag", "nonorm") and c.h_form in (None, "eye")


def obs_kernel(c):
    """launch_obs: k_obs_nd + k_obs_fin above D = 64 (the context has the per-observation buffer), else k_obs<false>"""
    return "k_obs_nd" if c.d > 64 else "k_obs"


def obs_times(m_obs, n_pts):
    """M = Np - 1: every index but 0 (adjacent, the last; row 0 is off the observations); M = 1: the last; else index 0 and the last
    M - 1 (adjacent, both boundaries) -- apart from index 0 of the third form, no index equals its counter (Q4)"""
    if m_obs == n_pts - 1:
        return np.arange(1, n_pts, dtype=np.int64)
    if m_obs == 1:
        return np.array([n_pts - 1], dtype=np.int64)
    return np.array([0] + list(range(n_pts - m_obs + 1, n_pts)), dtype=np.int64)


def obs_model(rng, d, r_form, h_form):
    if d == 1:
        return (0.04 if r_form == "diag" else 1.0 / (2.0 * np.pi)), (SCALAR_H if h_form == "scalar" else None)
    r = {"diag": lambda: np.diag(rng.uniform(0.5, 2.0, d)), "dense": lambda: xr.spd_with_spectrum(rng, d, 1e4, top=2.0),
         "nonorm": lambda: np.eye(d) / (2.0 * np.pi)}[r_form]()
    h = {None: lambda: None, "eye": lambda: np.eye(d), "noise": lambda: np.eye(d) + 0.1 * rng.standard_normal((d, d)),
         "mask": lambda: np.diag((np.arange(d) % 2 == 0).astype(float))}[h_form]()
    return r, h


def obs_problem(d, n_pts, obs_t, y, r, h):
    """an oracle problem that carries the observation model alone (eobs / eobs_gradients / xr.obs_terms read nothing else)"""
    return vo.Problem(model="OU" if d == 1 else "L96", method="euler", dt=DT, theta=1.0, sigma=None, m0=None, s0=None, mu0=None, tau0=None,
                      obs_t=np.asarray(obs_t, dtype=np.int64), obs_y=y, obs_noise=r, n_pts=n_pts, dim_d=d, obs_h=h)


def obs_state(rng, d, n_pts, obs_t, y, scale):
    """(m, S): m[t_n] = y_n (1 - scale u), |u| in [0.5, 1.5]; S_t SPD, its size different at every grid point (so that Q4 shows)"""
    if d == 1:
        m, s = rng.standard_normal(n_pts), rng.uniform(0.1, 0.4, n_pts)
        m[obs_t] = y * (1.0 - scale * _signed(rng, 0.5, 1.5, y.shape))
        return m, s
    m = 8.0 + rng.standard_normal((n_pts, d))
    m[obs_t] = y * (1.0 - scale * _signed(rng, 0.5, 1.5, y.shape))
    base = spd(rng, d, 0.2, 0.3)
    s = np.stack([_sym(base * u) for u in rng.uniform(0.5, 2.0, n_pts) * (1.0 + np.arange(n_pts) % 3)])
    return m, s


@functools.lru_cache(maxsize=None)
def obs_inputs(c):
    """(problem, m, S) of the case; an explicit identity shares every other input with H = None (they are compared bit for bit)"""
    h_seed = 0 if c.h_form in (None, "eye") else H_FORMS.index(c.h_form)
    rng = np.random.default_rng([c.d, c.m_obs, R_FORMS.index(c.r_form), h_seed, O_SCALES.index(c.scale) if c.scale in O_SCALES else 9])
    obs_t = obs_times(c.m_obs, c.n_pts)
    y = _signed(rng, 0.5, 1.5, c.m_obs) if c.d == 1 else 8.0 + rng.standard_normal((c.m_obs, c.d))
    m, s = obs_state(rng, c.d, c.n_pts, obs_t, y, c.scale)
    r, h = obs_model(rng, c.d, c.r_form, None if c.h_form == "eye" else c.h_form)
    return obs_problem(c.d, c.n_pts, obs_t, y, r, np.eye(c.d) if c.h_form == "eye" else h), m, s


def _obs_dicts(p, m, s):
    e, jm, js, parts = xr.obs_terms(p, m, s, parts=True)
    gm, gs = vo.eobs_gradients(p, m, s)
    kappas = {"Eobs": xr.kappa(np.concatenate((np.ravel(parts["terms"]), np.ravel(parts["const"]))))}
    return dict(Eobs=e, jm=jm, js=js), dict(Eobs=vo.eobs(p, m, s), jm=gm, js=gs), kappas, parts


@functools.lru_cache(maxsize=None)
def obs_reference(c):
    """(restatement, oracle, kappas, parts): once per session"""
    return _obs_dicts(*obs_inputs(c))


WORST_OBS = {}


@pytest.mark.parametrize("c", OBS_CASES, ids=case_id)
def test_observation_case_is_in_its_regime_and_the_reference_holds(c):
    p, m, s = obs_inputs(c)
    obs_t = np.asarray(p.obs_t)
    assert obs_t.size == c.m_obs and np.all(np.diff(obs_t) > 0) and 0 <= obs_t[0] and obs_t[-1] == c.n_pts - 1
    assert np.sum(obs_t != np.arange(c.m_obs)) >= c.m_obs - 1 and np.any(obs_t != np.arange(c.m_obs))
    if c.m_obs > 1:
        assert np.any(np.diff(obs_t) == 1)                      # adjacent indices
    off = np.abs(np.asarray(p.obs_y) - m[obs_t]) / np.abs(np.asarray(p.obs_y))
    assert np.all((0.4 * c.scale <= off) & (off <= 1.6 * c.scale)), (off.min(), off.max())
    ext, orc, kappas, parts = obs_reference(c)
    if c.d > 1:
        r = np.asarray(p.obs_noise)
        lam = np.linalg.eigvalsh(r)
        assert lam[0] > 0 and np.array_equal(r, r.T)            # no input leaves R indefinite
        for st in s:
            assert np.linalg.eigvalsh(st)[0] > 0 and np.array_equal(st, st.T)
        if c.r_form == "dense":
            assert abs(lam[-1] / lam[0] / 1e4 - 1.0) < 1e-6 and np.count_nonzero(r) == c.d ** 2
        if c.r_form == "diag":
            assert len(set(np.diag(r))) == c.d and np.count_nonzero(r) == c.d
        if c.h_form == "mask":
            assert np.linalg.matrix_rank(p.obs_h) == (c.d + 1) // 2
        # Q4: E_obs with S[t_n] where the oracle and the kernels read S[n] lies outside the bound of this case
        swapped = xr.obs_terms(p, m, s, q4=False)[0]
        moved, lim = ld_rel_err(swapped, ext["Eobs"]), kbound(ld_rel_err(orc["Eobs"], ext["Eobs"]), kappas["Eobs"])
        print(f"[obs {case_id(c)}] S[t_n] for S[n] moves E_obs by {moved:.2e} (bound {lim:.2e})")
        assert moved > lim
    if c.r_form == "nonorm":                                   # no normalisation constant: the per-observation terms alone
        assert abs(parts["const"]) <= 1e-14 * abs(ext["Eobs"])
        # the variance part of E_obs with R^-1 = 2 pi I: pi sum_n tr S[n] (1-D: pi sum_n s[t_n]); what is left is the data-fit sum
        var = np.asarray(s, dtype=LD)[obs_t] if c.d == 1 else np.asarray(np.einsum("tii->ti", s), dtype=LD)[:c.m_obs]
        fit = 1.0 - float(np.sum(var) * LD(np.pi) / ext["Eobs"])
        print(f"[obs {case_id(c)}] share of the data-fit sum in E_obs {fit:.2e}")
        assert 0.0 < fit < 1.0 and (fit > 0.5) == (c.scale == 1.0)
    self_check(f"[obs {case_id(c)}]", ext, orc, kappas, WORST_OBS)
    jm, js = np.asarray(ext["jm"]), np.asarray(ext["js"])
    rows_off = np.setdiff1d(np.arange(c.n_pts), obs_t)
    assert rows_off.size == c.n_pts - c.m_obs and not np.any(jm[rows_off]) and not np.any(js[rows_off])


def test_observation_table_meets_the_coverage_conditions():
    assert {(c.d, c.m_obs) for c in OBS_CASES if c.d == 1} == {(1, 1), (1, 256), (1, 257)}
    scalar = [c for c in OBS_CASES if c.h_form == "scalar"]                       # a 1-D operator h != 1: E_obs ignores it, the vector jump does not
    assert [(c.d, c.m_obs) for c in scalar] == [(1, 257)] and obs_inputs(scalar[0])[0].obs_h == SCALAR_H != 1.0
    assert all(c.n_pts == c.m_obs + 1 for c in OBS_CASES if c.d == 1)
    assert {(c.d, c.m_obs, c.n_pts) for c in OBS_CASES if 1 < c.d <= 64} == set(ND_SHAPES)
    assert (85 * 3 < 256 < 86 * 3) and 12 * 22 > 256 and 64 * 5 > 256          # the strided loop u < M D of k_obs on both sides of one pass
    for d, m, n in ND_SHAPES + LARGE_SHAPES:                                      # the diagonal and the dense branch at every shape
        assert {takes_diag_branch(c) for c in OBS_CASES if (c.d, c.m_obs) == (d, m)} == {False, True}, (d, m)
    assert {(c.r_form, c.h_form) for c in OBS_CASES if (c.d, c.m_obs, c.r_form != "nonorm") == (3, 86, True)} == set(ALL_FORMS)
    for d, m, n in ND_SHAPES:                                                     # an explicit identity beside H = None, every other input the same
        a, b = ObsCase(d, m, n, "diag", None, 0.1), ObsCase(d, m, n, "diag", "eye", 0.1)
        assert a in OBS_CASES and b in OBS_CASES
        (pa, ma, sa), (pb, mb, sb) = obs_inputs(a), obs_inputs(b)
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb) and np.array_equal(pa.obs_noise, pb.obs_noise) and pa.obs_h is None
        assert np.array_equal(pb.obs_h, np.eye(d))
    assert {(c.d, c.m_obs) for c in OBS_CASES if c.d > 64} == {(d, m) for d in (72, 257) for m in (1, 3)}
    assert 72 % 64 and 257 % 64 and 257 > 256                                    # j += 64 ragged at both D; i += 256 crossed at D = 257
    assert {(c.d, c.scale) for c in OBS_CASES if c.r_form == "nonorm"} == {(d, sc) for d in (1, 3) for sc in O_SCALES}
    assert len(OBS_CASES) == len(set(OBS_CASES))
    print("worst err_o, observation terms:", {q: f"{e:.1e}" for q, e in WORST_OBS.items()})


# ---- the per-problem observation model (k_obs<true>, k_obs_dense<true>) ----------------------------------------------------
ObsPmCase = collections.namedtuple("ObsPmCase", "model capacity n_pts batch form")
OBS_PM_CASES = [ObsPmCase(model, 4, 7, batch, form) for model, forms in (("OU", ("diag",)), ("L63", ("diag", "dense")))
                for batch in (3, 66) for form in forms]


def pm_count(c, k):
    """ragged counts: the smallest the header allows, the capacity, and one between"""
    return (1, c.capacity, c.capacity - 1)[k % 3]


@functools.lru_cache(maxsize=None)
def obs_pm_inputs(c, k):
    """problem k: (problem on its own count / R_k / H_k, m, S, the padded rows obs_t (capacity,), obs_y (capacity, D))"""
    d = MODEL_D[c.model]
    rng = np.random.default_rng([d, c.capacity, ("diag", "dense").index(c.form), 11, k])
    rows_t = np.sort(rng.choice(c.n_pts, c.capacity, replace=False)).astype(np.int64)
    if k == 0:
        rows_t = np.array([0, 1, c.n_pts - 2, c.n_pts - 1], dtype=np.int64)
    rows_y = _signed(rng, 0.5, 1.5, c.capacity) if d == 1 else 8.0 + rng.standard_normal((c.capacity, d))
    m, s = obs_state(rng, d, c.n_pts, rows_t, rows_y, 0.1)
    if d == 1:
        r, h = 0.04 * (1.0 + 0.01 * k), SCALAR_H            # (1-D models take no per-problem operator: the batch shares h != 1)
    else:
        r, h = obs_model(rng, d, c.form, "noise" if c.form == "dense" else None)
    n = pm_count(c, k)
    return obs_problem(d, c.n_pts, rows_t[:n], rows_y[:n], r, h), m, s, rows_t, rows_y


@functools.lru_cache(maxsize=None)
def obs_pm_reference(c, k):
    p, m, s, _, _ = obs_pm_inputs(c, k)
    return _obs_dicts(p, m, s)


@pytest.mark.parametrize("c", OBS_PM_CASES, ids=case_id)
def test_per_problem_observation_case_and_its_reference(c):
    assert {pm_count(c, k) for k in checked(c.batch)} >= {1, c.capacity} or c.batch < 64
    assert {pm_count(c, k) for k in range(3)} == {1, c.capacity, c.capacity - 1}
    seen = []
    for k in checked(c.batch):
        p, m, s, rows_t, rows_y = obs_pm_inputs(c, k)
        assert np.all(np.diff(rows_t) > 0) and 0 <= rows_t[0] and rows_t[-1] < c.n_pts
        if MODEL_D[c.model] > 1:
            assert np.linalg.eigvalsh(p.obs_noise)[0] > 0 and (p.obs_h is None) == (c.form == "diag")
        else:
            assert p.obs_h == SCALAR_H
        seen.append(np.ravel(p.obs_noise))
        ext, orc, kappas, _ = obs_pm_reference(c, k)
        self_check(f"[obs-pm {case_id(c)}] k={k}", ext, orc, kappas, WORST_OBS)
    assert len({tuple(v) for v in seen}) == len(seen)          # a different R_k per compared problem


# --------------------------------------------------------------------------- #
#  dF/dtheta behind a fused evaluation: Context.free_energy(x); Context.theta_gradient()
# --------------------------------------------------------------------------- #
ThetaCase = collections.namedtuple("ThetaCase", "path model n_pts batch flag own regime")
T_REGIMES = ("benign", "moments", "residual", "sign")
LANE_NPTS = {"OU": (2, 3, 4, 16, 17, 33), "DW": (2, 3, 4, 16, 17, 33), "L63": (2, 3, 4, 5, 9)}      # prefetch clamps; chunk edges T = 16 / 4


def _theta_cases():
    """lane: k_theta_lane -- every Np (regimes rotate, B = 1 for the 1-D models and 520 for Lorenz-63), then B = 63, 64, 65 at Np = 17, the
    last with per-problem theta.  hyp: the hyp_only launches + k_trapz_multi -- Lorenz-63 on 16 lanes per problem (B = 5), the four-kernel
    path (FLAG_MATERIALIZE) and the generic steppers (FLAG_FORCE_GENERIC); Np = 2, 257, 258 for the 1-D models, 2 and 65 for Lorenz-63."""
    cases = []
    for model in MODELS:
        nb = 520 if model == "L63" else 1
        for i, n in enumerate(LANE_NPTS[model]):
            cases.append(ThetaCase("lane", model, n, nb, None, model == "L63" and i == 4, T_REGIMES[i % 4]))
        if model != "L63":
            cases += [ThetaCase("lane", model, 17, b, None, b == 65, T_REGIMES[j]) for j, b in enumerate((63, 64, 65))]
            cases.append(ThetaCase("lane", model, 33, 65, None, False, "sign"))
    for j, (model, flag, nb) in enumerate((("L63", None, 5), ("OU", "FLAG_MATERIALIZE", 2), ("DW", "FLAG_MATERIALIZE", 2), ("L63", "FLAG_MATERIALIZE", 520),
                                           ("DW", "FLAG_FORCE_GENERIC", 2), ("L63", "FLAG_FORCE_GENERIC", 2))):
        for i, n in enumerate((2, 65) if model == "L63" else (2, 257, 258)):
            cases.append(ThetaCase("hyp", model, n, nb, flag, (i + j) % 2 == 1, T_REGIMES[(i + j) % 4] if n > 2 else T_REGIMES[j % 3]))
    return cases


THETA_CASES = _theta_cases()


@functools.lru_cache(maxsize=None)
def theta_problem(model, n_pts, regime):
    """The oracle problem of a case (shared by its batch) and the x of problem 0.  benign: make_problem.  moments / residual: the sweep
    starts at an m0, s0 of the energy regime of the same name and b_t = A_t m0 + ... holds the mean there.  sign: b_t alternates, so
    that the integrand of dF/dtheta changes sign along the grid and kappa is above 1."""
    d, single = MODEL_D[model], model in ("OU", "DW")
    p, x = make_problem(model, d, n_pts, method="rk4", obs_at=sorted({0, n_pts - 1} if n_pts < 4 else {1, n_pts - 2}))
    if regime == "benign":
        return p, x
    if regime == "sign" and single:                              # the benign problem with b_t = +6, -6, +6, ...: m_t b_t dominates the integrand
        return p, np.concatenate((x[:n_pts], np.where(np.arange(n_pts) % 2 == 0, 6.0, -6.0)))
    rng = np.random.default_rng([MODELS.index(model), n_pts, T_REGIMES.index(regime), 13])
    small = 1e-3 if regime == "residual" else 1.0
    if single:
        theta, sigma = (1.3 if model == "OU" else 1.0), 0.8 * small
        m0 = float(_signed(rng, 1.2, 1.8, 1)[0]) if model == "DW" else float(_signed(rng, 0.5, 1.5, 1)[0])
        s0 = small * (0.8 if model == "DW" else 0.9)
        a = _signed(rng, 0.5, 2.0, n_pts)
        hold_m = a * m0                                          # b = A m: dm/dt = 0
    else:
        theta, sigma = np.array([1.3, 0.9, 1.1]), small * np.diag([0.8, 1.0, 1.2])
        m0 = _signed(rng, 0.5, 1.0, 3)
        dv = rng.uniform(0.9, 1.1, 3)
        s0 = small * _sym(dv[:, None] * L63_CORR * dv[None, :])
        a = 5.0 * rng.standard_normal((n_pts, 3, 3))
        hold_m = a.dot(m0)
    p = dataclasses.replace(p, theta=theta, sigma=sigma, m0=m0, s0=s0, obs_y=np.asarray(p.obs_y) * 0.0 + (m0 if single else m0[None, :]) * 1.01)
    if regime == "moments":
        b = hold_m + _signed(rng, 0.5, 1.5, np.shape(hold_m))
    elif regime == "residual":
        shape = (n_pts,) if single else (n_pts, 3)
        mm = np.full(shape, m0) if single else np.tile(m0, (n_pts, 1))
        ss = np.full(shape, s0) if single else np.tile(s0, (n_pts, 1, 1))
        b = _mean_drift(model, theta, mm, ss) + hold_m - 1e-3 * _signed(rng, 0.5, 1.5, shape)
    else:
        sgn = np.where(np.arange(n_pts) % 2 == 0, 1.0, -1.0)
        b = hold_m + (3.0 * sgn if single else 3.0 * sgn[:, None] * np.ones(3))
    return p, np.concatenate((np.ravel(a), np.ravel(b)))


@functools.lru_cache(maxsize=None)
def theta_inputs(c, k):
    """(problem, x) of problem k: its own x, and its own theta where c.own"""
    p, x = theta_problem(c.model, c.n_pts, c.regime)
    rng = np.random.default_rng([MODELS.index(c.model), c.n_pts, T_REGIMES.index(c.regime), 17, k])
    x = x * (1.0 + 1e-3 * rng.standard_normal(x.size))
    if c.own:
        th = np.asarray(p.theta, dtype=float) * (1.0 + 0.02 * (k % 7 + 1))
        p = dataclasses.replace(p, theta=float(th) if th.ndim == 0 else th)
    return p, x


@functools.lru_cache(maxsize=None)
def theta_reference(c, k):
    """(restatement, oracle, kappas) of dF/dtheta of problem k, dicts over ("dFdth",): once per session"""
    p, x = theta_inputs(c, k)
    a, b = p.split(x)
    mt, st = xr.solve_fwd(p.method, p.dt, a, b, p.m0, p.s0, p.sigma)
    val, kap = xr.theta_gradient(p, x, dict(mt=mt, st=st))
    _, state = vo.free_energy(p, x, faithful=False)
    return dict(dFdth=val), dict(dFdth=np.atleast_1d(state["dEsde_dth"])), dict(dFdth=kap)


WORST_THETA = {}


@pytest.mark.parametrize("c", THETA_CASES, ids=case_id)
def test_theta_case_is_in_its_regime_and_the_reference_holds(c):
    for k in checked(c.batch):
        p, x = theta_inputs(c, k)
        with np.errstate(over="raise", invalid="raise", divide="raise"):
            _, state = vo.free_energy(p, x, faithful=False)
        for st in np.reshape(state["st"], (c.n_pts, MODEL_D[c.model], -1)):
            assert np.linalg.eigvalsh(_sym(st))[0] > 0            # no input leaves S_t indefinite
        ext, orc, kappas = theta_reference(c, k)
        self_check(f"[theta {case_id(c)}] k={k}", ext, orc, kappas, WORST_THETA)
        if c.regime == "sign" and c.n_pts > 2:
            assert np.max(kappas["dFdth"]) > 1.05, kappas          # (kappa > 1: the integrand changes sign along the grid)
    if c.own:
        assert theta_inputs(c, 0)[0].theta is not theta_inputs(c, c.batch - 1)[0].theta
        assert not np.array_equal(theta_inputs(c, 0)[0].theta, theta_inputs(c, c.batch - 1)[0].theta)


def test_lorenz96_branch_of_the_restated_theta_gradient():
    """xr.theta_gradient on a Lorenz-96 problem (no GPU case of this module calls it: test_l96_energy_conditioning holds that kernel): the
    difference quotient of the restated E_sde equals the integral of the unscented mean residual that energy_l96 returns."""
    p, x = make_problem("L96", 12, 6)
    a, b = p.split(x)
    mt, st = xr.solve_fwd(p.method, p.dt, a, b, p.m0, p.s0, p.sigma)
    val, kap = xr.theta_gradient(p, x, dict(mt=mt, st=st))
    want = xr.energy_l96(p.theta, p.sigma, p.dt, a, b, mt, st)["theta_integral"]
    assert val.shape == kap.shape == (1,) and val.dtype == LD and kap[0] >= 1.0
    assert ld_rel_err(val[0], want) <= 1e-16


def test_theta_table_meets_the_coverage_conditions():
    lane, hyp = [c for c in THETA_CASES if c.path == "lane"], [c for c in THETA_CASES if c.path == "hyp"]
    for model in MODELS:
        assert {c.n_pts for c in lane if c.model == model} == set(LANE_NPTS[model])
    assert {c.batch for c in lane if c.model in ("OU", "DW")} == {1, 63, 64, 65} and {c.batch for c in lane if c.model == "L63"} == {520}
    assert {c.own for c in lane if c.model == "L63"} == {c.own for c in lane if c.model == "OU"} == {False, True}
    assert {(c.model, c.flag, c.batch) for c in hyp} == {("L63", None, 5), ("OU", "FLAG_MATERIALIZE", 2), ("DW", "FLAG_MATERIALIZE", 2),
                                                         ("L63", "FLAG_MATERIALIZE", 520), ("DW", "FLAG_FORCE_GENERIC", 2), ("L63", "FLAG_FORCE_GENERIC", 2)}
    assert {c.n_pts for c in hyp if c.model != "L63"} == {2, 257, 258} and {c.n_pts for c in hyp if c.model == "L63"} == {2, 65}
    assert {c.own for c in hyp} == {False, True}
    for model in MODELS:                                       # every regime per model, and a sign-changing integrand per model
        assert {c.regime for c in THETA_CASES if c.model == model} == set(T_REGIMES), model
    assert len(THETA_CASES) == len(set(THETA_CASES))
    print("worst err_o, dF/dtheta:", {q: f"{e:.1e}" for q, e in WORST_THETA.items()})


# --------------------------------------------------------------------------- #
#  Fused paths of the small models other than the lane pass (the cases are test_stepper_rounding_cpu.FusedCase: its references serve)
# --------------------------------------------------------------------------- #
SMALL_PATHS = (("wave63", "L63", 5, None), ("materialize", "OU", 2, "FLAG_MATERIALIZE"), ("materialize", "DW", 2, "FLAG_MATERIALIZE"),
               ("materialize", "L63", 520, "FLAG_MATERIALIZE"), ("generic_small", "DW", 2, "FLAG_FORCE_GENERIC"),
               ("generic_small", "L63", 2, "FLAG_FORCE_GENERIC"))
SMALL_FUSED_CASES = [FusedCase(f, model, MODEL_D[model], 12, ("rk4", "heun", "rk2", "euler")[(i + r) % 4], b, flag, "diag", regime)
                     for i, (f, model, b, flag) in enumerate(SMALL_PATHS) for r, regime in enumerate(("benign", "near"))]
WORST_SMALL = {}


@functools.lru_cache(maxsize=None)
def small_fused_drift(c, k):
    """(restatement, oracle) of <f> and <df/dx> of problem k, dicts over (Efx, Edf): what vgpa_fetch serves with k_edf_dense"""
    p, _ = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    a, b = p.split(fused_x(c, k))
    ext, orc = fused_reference(c, k)
    en = xr.model_energy(p, a, b, ext["mt"], ext["st"])
    _, (ef, edf), _ = vo.model_energy(p, a, b, np.asarray(orc["mt"]), np.asarray(orc["st"]), faithful=False)
    return dict(Efx=en["Ef"], Edf=en["Edf"]), dict(Efx=ef, Edf=edf)


@pytest.mark.parametrize("c", SMALL_FUSED_CASES, ids=case_id)
def test_small_fused_case_reference_holds(c):
    """the regimes are test_stepper_rounding_cpu's (fused_x, near_optimum: NEAR_DROP is asserted here for these problems too)"""
    p, x0 = fused_problem(c.model, c.d, c.n_pts, c.method, c.sigma)
    for k in checked(c.batch):
        if c.regime == "near":
            assert glb_max(p, fused_x(c, k)) <= glb_max(p, x0) / NEAR_DROP
        self_check(f"[fused {case_id(c)}] k={k} drift", *small_fused_drift(c, k), {}, WORST_SMALL)
        ext, orc = fused_reference(c, k)
        for q in ext:
            err_o = ld_rel_err(orc[q], ext[q])
            WORST_SMALL[q] = max(WORST_SMALL.get(q, 0.0), err_o)
            assert 0.0 <= err_o <= RESTATEMENT_TOL, (c, k, q, err_o)
    assert {(f, m) for f, m, *_ in SMALL_PATHS} == {(c.family, c.model) for c in SMALL_FUSED_CASES}


# ---- fused sweeps with an observation model that is not R = I, H = I ----------------------------------------------------------
# pm: every problem has its own count (1, 3, 2, 1, ...), R_k and H_k (vgpa_set_problem_obs_model); else the batch shares one model.
FusedObsCase = collections.namedtuple("FusedObsCase", "family model d n_pts method batch flag sigma form pm")
FUSED_OBS_CASES = (
    [FusedObsCase(f, model, MODEL_D[model], 12, "rk4", b, flag, "diag", "dense", False) for f, model, b, flag in SMALL_PATHS] +
    [FusedObsCase("lane_pass", "OU", 1, 12, "rk4", 3, None, "diag", "dense", False)] +
    [FusedObsCase("packed", "L96", 36, 6, "rk4", 3, None, "iso", form, False) for form in ("diag", "dense")] +
    [FusedObsCase("lane_pass", "OU", 1, 12, "rk4", b, None, "diag", "diag", True) for b in (3, 66, 130)] +
    [FusedObsCase("wave63", "L63", 3, 12, "rk4", b, None, "diag", "dense", True) for b in (3, 66)] +
    [FusedObsCase("lane_pass", "L63", 3, 12, "rk4", 520, None, "diag", form, True) for form in ("diag", "dense")])
FUSED_OBS_LANE = ("F", "gLa", "gLb", "Esde", "Eobs", "mt", "st")


def fused_obs_quantities(c):
    """what a case compares: everything vgpa_fetch serves from the arrays the sweep left; on the lane pass, whose lam_t and Psi_t exist only
    as the separate kernels' (test_stepper_rounding.test_fused_lane_pass), what the pass itself computes"""
    return FUSED_OBS_LANE if c.family == "lane_pass" else FUSED_QUANTITIES


def fused_obs_kernel(c):
    """which observation kernel the case runs, by the rule of the fused entry points: the lane pass has its own (k_obs_lane<D, PM>); every
    other context goes through launch_obs (k_obs<PM> up to D = 64)"""
    return f"k_obs_lane<{c.d}, {str(c.pm).lower()}>" if c.family == "lane_pass" else f"k_obs<{str(c.pm).lower()}>"


@functools.lru_cache(maxsize=None)
def fused_obs_problem(c, k):
    """(problem k on its own count / R_k / H_k, its x, the base problem whose three observations are the rows of every problem).  1-D
    models: r = 0.07 (per problem: 0.04 (1 + 0.01 k)) and the scalar operator h = 1.3, which a batch always shares."""
    n = c.n_pts
    base, x = make_problem(c.model, c.d, n, method=c.method, obs_at=[1, n // 2, n - 1], sigma=c.sigma)
    own = k if c.pm else 0
    rng = np.random.default_rng([c.d, n, ("diag", "dense").index(c.form), 19, own])
    if c.d == 1:
        r, h = (0.04 * (1.0 + 0.01 * own) if c.pm else 0.07), SCALAR_H
    else:
        r, h = obs_model(rng, c.d, c.form, "noise" if c.form == "dense" else None)
    cnt = (1, 3, 2)[k % 3] if c.pm else 3
    p = dataclasses.replace(base, obs_t=base.obs_t[:cnt], obs_y=base.obs_y[:cnt], obs_noise=r, obs_h=h)
    xk = x + (0.05 if c.d <= 3 else 0.02) * np.random.default_rng([c.d, n, 23, k]).standard_normal(x.size)
    return p, xk, base


@functools.lru_cache(maxsize=None)
def fused_obs_reference(c, k):
    """(restatement, oracle, kappas) of problem k, dicts over fused_obs_quantities(c): once per session"""
    p, x, _ = fused_obs_problem(c, k)
    f, gla, glb, state = xr.sweep(p, x, float(np.asarray(vo.kl0(p))))
    f_o, g_o, st_o = vo.sweep(p, x, faithful=False)
    parts = xr.obs_terms(p, state["mt"], state["st"], parts=True)[3]
    kappas = {"Eobs": xr.kappa(np.concatenate((np.ravel(parts["terms"]), np.ravel(parts["const"]))))}
    ext, orc = fused_quantities(p, f, np.concatenate((gla, glb)), state), fused_quantities(p, f_o, g_o, st_o)
    return {q: ext[q] for q in fused_obs_quantities(c)}, {q: orc[q] for q in fused_obs_quantities(c)}, kappas


@pytest.mark.parametrize("c", FUSED_OBS_CASES, ids=case_id)
def test_fused_observation_case_and_its_reference(c):
    seen = []
    for k in checked(c.batch):
        p, x, base = fused_obs_problem(c, k)
        assert list(base.obs_t) == [1, c.n_pts // 2, c.n_pts - 1] and np.all(base.obs_t != np.arange(3))      # Q4 shows
        assert np.array_equal(p.obs_t, base.obs_t[:p.obs_t.size]) and p.obs_t.size == ((1, 3, 2)[k % 3] if c.pm else 3)
        if c.d > 1:
            assert np.linalg.eigvalsh(p.obs_noise)[0] > 0 and (p.obs_h is not None) == (c.form == "dense")
            assert (np.count_nonzero(p.obs_noise) == c.d) == (c.form == "diag")
        else:
            assert p.obs_h == SCALAR_H != 1.0 and p.obs_noise != 1.0
        seen.append(tuple(np.ravel(p.obs_noise)))
        ext, orc, kappas = fused_obs_reference(c, k)
        self_check(f"[fused-obs {case_id(c)}] k={k}", ext, orc, kappas, WORST_SMALL)
    assert (len(set(seen)) == len(seen)) == (c.pm or len(seen) == 1)
    if c.pm:
        assert {(1, 3, 2)[k % 3] for k in checked(c.batch)} >= {1, 3} or c.batch == 3


def test_fused_tables_meet_the_coverage_conditions():
    assert {(c.family, c.model) for c in SMALL_FUSED_CASES} == {(f, m) for f, m, *_ in SMALL_PATHS}
    for f, m, *_ in SMALL_PATHS:
        assert {c.regime for c in SMALL_FUSED_CASES if (c.family, c.model) == (f, m)} == {"benign", "near"}
    shared = [c for c in FUSED_OBS_CASES if not c.pm]
    assert {(c.family, c.model, c.batch, c.flag) for c in shared if c.family in ("wave63", "materialize", "generic_small")} == set(SMALL_PATHS)
    assert all(c.form == "dense" and c.n_pts == 12 for c in shared if c.family != "packed")      # every fused path: dense R / non-identity H (1-D: r, h != 1)
    assert [c.batch for c in shared if c.family == "lane_pass"] == [3]
    assert {c.form for c in shared if c.family == "packed"} == {"diag", "dense"} and all(c.d == 36 and c.sigma == "iso" for c in shared if c.family == "packed")
    pm = [c for c in FUSED_OBS_CASES if c.pm]
    assert {c.batch for c in pm if c.model == "OU"} == {3, 66, 130} and {c.batch for c in pm if c.model == "L63"} == {3, 66, 520}
    assert {fused_obs_kernel(c) for c in FUSED_OBS_CASES} == {"k_obs<false>", "k_obs<true>", "k_obs_lane<1, false>", "k_obs_lane<1, true>", "k_obs_lane<3, true>"}
    assert len(FUSED_OBS_CASES) == len(set(FUSED_OBS_CASES)) and len(SMALL_FUSED_CASES) == len(set(SMALL_FUSED_CASES))
    print("worst err_o, fused small paths:", {q: f"{e:.1e}" for q, e in WORST_SMALL.items()})


# --------------------------------------------------------------------------- #
#  The bound closes the gap: mutants of the oracle's expressions
# --------------------------------------------------------------------------- #
def _l63_point_mutant(theta, at, bt, mt, st, isg, cross=2):
    """The third component of vo.l63_point's <(f - g)^2>, restated from the oracle's text with `cross` S_xy^2 in E[x^2 y^2] (the oracle: 2);
    the other two components are the oracle's.  Returns Efg alone: the gradients and E[x^2 z^2] stay unmutated."""
    efg, _, _ = vo.l63_point(theta, at, bt, mt, st, isg)
    vB = theta[2]
    A31, A32, A33 = at[2]
    b3 = bt[2]
    mx, my, mz = mt
    Sxx, Sxy, Sxz = st[0]
    Syy, Syz = st[1][1], st[1][2]
    Szz = st[2][2]
    Exx, Exy, Exz = Sxx + mx ** 2, Sxy + mx * my, Sxz + mx * mz
    Eyy, Eyz, Ezz = Syy + my ** 2, Syz + my * mz, Szz + mz ** 2
    Exxy = Sxx * my + 2 * Sxy * mx + (mx ** 2) * my
    Exyy = Syy * mx + 2 * Sxy * my + (my ** 2) * mx
    Exyz = Sxy * mz + Sxz * my + Syz * mx + mx * my * mz
    Exxyy = Sxx * (my ** 2 + Syy) + Syy * (mx ** 2) + 4.0 * Sxy * mx * my + (mx * my) ** 2 + cross * (Sxy ** 2)
    EZ = Exxyy + (vB ** 2) * Ezz + (A31 ** 2) * Exx + (A32 ** 2) * Eyy + (A33 ** 2) * Ezz + \
        b3 ** 2 + 2 * (A31 * Exxy + A32 * Exyy + A33 * Exyz + A31 * A32 * Exy +
                       A31 * A33 * Exz + A32 * A33 * Eyz -
                       vB * (Exyz + A31 * Exz + A32 * Eyz + A33 * Ezz) -
                       b3 * (Exy - vB * mz + A31 * mx + A32 * my + A33 * mz))
    return np.array([efg[0], efg[1], EZ])


def _esde_l63(theta, sigma, a, b, m, s, cross):
    isg = np.diag(vo.chol_inv(sigma)[0])
    e_t = np.array([0.5 * isg.dot(_l63_point_mutant(theta, a[t], b[t], m[t], s[t], isg, cross)) for t in range(m.shape[0])])
    return vo.my_trapz(e_t, DT, [])


def _esde_dw(theta, sigma, a, b, m, s, eps):
    c = (4.0 * theta) + a
    ex6 = m ** 6 + 15 * (m ** 4) * s + 45 * (m ** 2) * (s ** 2) + 15 * (s ** 3) * (1.0 + eps)
    var_q = 8.0 * (ex6 - c * vo.gm(m, s, 4) + b * vo.gm(m, s, 3)) + ((c ** 2) * vo.gm(m, s, 2)) - (2.0 * b * c * m) + (b ** 2)
    return 0.5 * vo.my_trapz(var_q, DT, []) / sigma


def _eobs_time_indexed(p, m, s):
    """vo.eobs (n-D) with S[t_n] for S[n]"""
    w = (p.obs_y - m[p.obs_t]).dot(vo._obs_operator(p))
    inv_r, inv_c = vo.chol_inv(p.obs_noise)
    z = w.dot(inv_c.T)
    s_diag = np.diagonal(s, axis1=1, axis2=2)
    acc = 0.0
    for n in range(p.obs_y.shape[0]):
        acc += np.inner(z[n], z[n]) + np.inner(inv_r.diagonal(), s_diag[p.obs_t[n]])
    return 0.5 * (acc + p.obs_y.shape[0] * (p.obs_y.shape[1] * vo.LOG2PI + vo.log_det(p.obs_noise)))


def _jump_hrh(p, m, transposed):
    """the vector jump of vo.eobs_gradients; transposed=False: H^T R^-1 H (y - m) in place of H^T R^-1 H^T (y - m)"""
    h = vo._obs_operator(p)
    w = (p.obs_y - m[p.obs_t]).dot(h) if transposed else (p.obs_y - m[p.obs_t]).dot(h.T)
    inv_r, _ = vo.chol_inv(p.obs_noise)
    jm = np.zeros(m.shape)
    for k, tn in enumerate(p.obs_t):
        jm[tn] = -h.T.dot(inv_r).dot(w[k])
    return jm


def _old_inputs_l63():
    """what the older tests feed the Lorenz-63 energy: the golden fixture and make_problem (benign), each with the oracle's (m_t, S_t)"""
    z = load_golden("l63_rk4_p")
    pg = vo.Problem.from_fixture(z)
    out = [(pg,) + tuple(pg.split(z["x"])) + (z["mt"], z["st"])]
    p, x = make_problem("L63", 3, 30)
    _, st = vo.free_energy(p, x, faithful=False)
    return out + [(p,) + tuple(p.split(x)) + (st["mt"], st["st"])]


def test_the_mutants_pass_the_old_check_and_miss_the_new_bound():
    """Four mutants of the oracle's expressions.  For each: the unmutated copy IS the oracle (bit for bit); whether the old check (1e-9
    against the oracle on the golden / make_problem inputs) lets it through is reported and, for the first two, asserted; on the new inputs
    it misses the bound of this module."""
    report = {}
    # 1. 2 Sxy^2 -> Sxy^2 in the Lorenz-63 fourth moment
    old = []
    for p, a, b, m, s in _old_inputs_l63():
        want = vo.energy_l63(p.theta, p.inverse_sigma, p.dt, a, b, m, s, [])[0]
        isg = np.diag(p.inverse_sigma)
        same = vo.my_trapz(np.array([0.5 * isg.dot(_l63_point_mutant(p.theta, a[t], b[t], m[t], s[t], isg, 2)) for t in range(m.shape[0])]), p.dt, [])
        got = vo.my_trapz(np.array([0.5 * isg.dot(_l63_point_mutant(p.theta, a[t], b[t], m[t], s[t], isg, 1)) for t in range(m.shape[0])]), p.dt, [])
        assert same == want
        old.append(abs(got - want) / abs(want))
    c = EnergyCase("L63", "moments", 65, 1, False, False)
    theta, sigma, a, b, m, s = energy_inputs(c, 0)
    ext, orc, _ = energy_reference(c, 0)
    assert _esde_l63(theta, sigma, a, b, m, s, 2) == orc["Esde"]
    err_o, err_k = ld_rel_err(orc["Esde"], ext["Esde"]), ld_rel_err(_esde_l63(theta, sigma, a, b, m, s, 1), ext["Esde"])
    report["l63 cross term"] = (max(old), err_o, err_k)
    assert max(old) < 1e-9 and not err_k <= bound(err_o)
    # 2. 15 s^3 -> 15 s^3 (1 + 2^-30) in the double-well sixth moment
    old = []
    z = load_golden("dw_rk4_p")
    pg = vo.Problem.from_fixture(z)
    p2, x2 = make_problem("DW", 1, 30)
    _, st2 = vo.free_energy(p2, x2, faithful=False)
    for p, (a_, b_), m_, s_ in ((pg, pg.split(z["x"]), z["mt"], z["st"]), (p2, p2.split(x2), st2["mt"], st2["st"])):
        want = vo.energy_dw(p.theta, p.sigma, DT, a_, b_, m_, s_, [])[0]
        assert _esde_dw(p.theta, p.sigma, a_, b_, m_, s_, 0.0) == want
        old.append(abs(_esde_dw(p.theta, p.sigma, a_, b_, m_, s_, 2.0 ** -30) - want) / abs(want))
    c = EnergyCase("DW", "moments", 257, 1, False, False)
    theta, sigma, a, b, m, s = energy_inputs(c, 0)
    ext, orc, _ = energy_reference(c, 0)
    assert _esde_dw(theta, sigma, a, b, m, s, 0.0) == orc["Esde"]
    err_o, err_k = ld_rel_err(orc["Esde"], ext["Esde"]), ld_rel_err(_esde_dw(theta, sigma, a, b, m, s, 2.0 ** -30), ext["Esde"])
    report["dw 15 s^3"] = (max(old), err_o, err_k)
    assert max(old) < 1e-9 and not err_k <= bound(err_o)
    # 3. S[t_n] instead of S[n] in E_obs; 4. H^T R^-1 H in place of H^T R^-1 H^T in the vector jump -- old inputs: make_problem(dense=True)
    # with a non-identity H (test_dense_noise_matrices_and_observation_operator) and the golden Lorenz-63 fixture (R diagonal, H = I)
    rng = np.random.default_rng(11)
    pd, xd = make_problem("L63", 3, 11, dense=True, h_op=np.eye(3) + 0.1 * rng.standard_normal((3, 3)), obs_at=[0, 4, 10])
    _, sd = vo.free_energy(pd, xd, faithful=False)
    zg = load_golden("l63_rk4_p")
    pg = vo.Problem.from_fixture(zg)
    old_q4, old_h = [], []
    for p, m_, s_ in ((pd, sd["mt"], sd["st"]), (pg, zg["mt"], zg["st"])):
        assert _eobs_time_indexed(dataclasses.replace(p, obs_t=np.arange(p.obs_t.size)), m_, s_) == \
            vo.eobs(dataclasses.replace(p, obs_t=np.arange(p.obs_t.size)), m_, s_)      # (index == counter: the same text, the same bits)
        assert np.array_equal(_jump_hrh(p, m_, True), vo.eobs_gradients(p, m_, s_)[0])
        old_q4.append(abs(_eobs_time_indexed(p, m_, s_) - vo.eobs(p, m_, s_)) / abs(vo.eobs(p, m_, s_)))
        old_h.append(rel_err(_jump_hrh(p, m_, False), vo.eobs_gradients(p, m_, s_)[0]))
    c = ObsCase(3, 86, 87, "dense", "noise", 0.1)
    p, m, s = obs_inputs(c)
    ext, orc, kappas, _ = obs_reference(c)
    err_o, err_k = ld_rel_err(orc["Eobs"], ext["Eobs"]), ld_rel_err(_eobs_time_indexed(p, m, s), ext["Eobs"])
    report["S[t_n] in E_obs"] = (tuple(old_q4), err_o, err_k)
    assert not err_k <= kbound(err_o, kappas["Eobs"])
    assert np.array_equal(_jump_hrh(p, m, True), orc["jm"])
    err_o, err_k = ld_rel_err(orc["jm"], ext["jm"]), ld_rel_err(_jump_hrh(p, m, False), ext["jm"])
    report["H^T R^-1 H jump"] = (tuple(old_h), err_o, err_k)
    assert not err_k <= bound(err_o)
    for name, (old, err_o, err_k) in report.items():
        print(f"[mutant {name}] old check: {old}; new inputs: err_o={err_o:.2e} err_k={err_k:.2e} ratio={ratio(err_k, err_o):.3g}")
    # what the old check does with the last two: S[t_n] is caught wherever an index differs from its counter; the transposed operator is
    # invisible where H = I (the golden fixture) and caught where H is not symmetric
    assert min(old_q4) > 1e-9 and min(old_h) == 0.0 and max(old_h) > 1e-9
