"""
The case tables, the references and the expected launches of test_large_d_rounding.py (GPU), checked without a device: every stage path
above D = 64 -- k_stage_prod, k_stage_wide, the two-kernel stage, the literal non-symmetric path, the batched drivers, VGPA_FLAG_LIBRARY_GEMM,
the row-sharded native driver, the fused sweep above D = 72 -- under the bound of test_stepper_rounding_cpu.py,

    err_k(q) <= FACTOR * max(err_o(q), 2^-53)                                                  FACTOR = 32

built from that module's own pieces (OpCase, FusedCase, op_shared, op_problem, op_reference, fused_problem, fused_x, fused_reference, bound,
ratio, ld_rel_err, checked, self_check); its tables and coverage assertions are untouched.  Every case here goes through that module's
two regime functions (benign rho dt < 0.1; stiff 0.4 <= rho dt <= 1, cond(S0) = 1e6, S_t positive definite, no overflow; near-optimum
gradient drop >= 20; oracle against restatement <= 1e-11).  A reference is keyed by what its inputs depend on -- (D, method, regime,
symmetry, problem) -- so the paths that run the same inputs share it.

Where a shape of the table could not be what it was meant to be, by the selection rule of large_d.hip::run_stage restated in `stage_path`:
  * D = 258 at one problem has 9 tiles = 45 tile pairs <= kStageProdMaxPairs and runs k_stage_prod; the same tile structure reaches
    k_stage_wide by the default rule at two problems (90 pairs): the unit is (258, batch 2).
  * The row-sharded driver forms its mid-point operand once per step with k_mid_cols and multiplies with the plain product: its serial
    schedule (chunks = 0) runs k_gemm_v, not the mid-point-averaging product.  That product (MID) is reached through vgpa_ld_gemm with a
    second operand only, and is tested there (GEMM_CASES).

`expected_launches` states, per case, which counters of vgpa_ld_launch_counts move and how far; `gemm_form` restates launch_gemm's score
and its choice of kernel form, so the shapes of GEMM_CASES are shown to select their tile height here, before a device is involved.

Measured here, on the CPU (worst err_o over the compared problems of each table; every case prints its own; every case was in its regime):
  operator level  benign: m_t 3.6e-16, S_t 5.0e-16, lam_t 1.7e-16, Psi_t 2.9e-16;  stiff: m_t 3.5e-16, S_t 2.3e-15, lam_t 2.7e-16, Psi_t 7.9e-16
  fused, near     F 8.0e-17, gLa 1.7e-14, gLb 1.4e-13, E_sde 1.5e-16, E_obs 9.1e-17, m_t 2.9e-16, S_t 2.5e-16, lam_t 1.5e-15, Psi_t 3.1e-15,
                  dEsde_dm 5.8e-15, dEsde_dS 5.0e-15
  fused, stiff    F 6.8e-17, gLa 5.6e-15, gLb 3.6e-15, E_sde 9.0e-17, E_obs 2.6e-16, m_t 2.6e-16, S_t 5.8e-16, lam_t 7.9e-15, Psi_t 8.5e-14,
                  dEsde_dm 1.0e-14, dEsde_dS 1.5e-13
  so oracle and restatement agree to 1.5e-13 at worst, against RESTATEMENT_TOL = 1e-11.
The mutant (fourth RK4 slope of S_t and of Psi_t times 1 + 2^-30) at D = 130 and D = 330, 5 grid points: against the oracle S_t 1.1e-11 ...
4.6e-11, Psi_t 2.2e-11 ... 1.3e-10 -- all pass 1e-9; err_k / max(err_o, 2^-53): S_t 4.4e4 ... 1.1e5, Psi_t 2.0e5 ... 4.4e5 -- three to four
decimal orders over FACTOR, at D = 330 as at D = 130.  The module takes 110 s, nearly all of it the longdouble references (D = 514 Heun
11 s, D = 384 RK4 8 s each, the 60 SCG iterations at D = 200 9 s).
"""
import collections

import numpy as np
import pytest

import test_stepper_rounding_cpu as base
from conftest import rel_err
from test_stepper_rounding_cpu import (FACTOR, METHODS, OP_QUANTITIES, OP_REGIMES, FusedCase, OpCase, bound, case_id, ld_rel_err,
                                       op_reference, ratio)
from vgpa_amd import _lib

N_PTS = 5
STAGES = {"euler": (1, 0), "heun": (2, 0), "rk2": (2, 1), "rk4": (4, 2)}       # stages of a step, and how many of them read the mid-point pair

# --------------------------------------------------------------------------- #
#  large_d.hip's selection rules, restated
# --------------------------------------------------------------------------- #
K_STAGE_PROD_MAX_D, K_STAGE_PROD_MAX_PAIRS, K_STAGE_WIDE_MAX_D, K_STAGE_WIDE_FULL_TILE_D = 512, 64, 2048, 384


def stage_path(d, batch=1, fused_env=None, wide_env=None, literal=False, library=False):
    """run_stage's rule: "prod", "wide" or "two" (the operands are 16-byte aligned and evenly strided wherever D is even)"""
    fused_ok = not library and not literal
    nt = (d + 31) // 32
    wide_max = K_STAGE_WIDE_MAX_D if wide_env is None else int(wide_env)
    prod_max = K_STAGE_PROD_MAX_D if fused_env is None else int(fused_env)
    wide = fused_ok and d % 2 == 0 and d <= wide_max and (d % 64 != 0 or d < K_STAGE_WIDE_FULL_TILE_D or wide_env is not None)
    if fused_ok and d <= prod_max and (nt * (nt + 1) // 2 * batch <= K_STAGE_PROD_MAX_PAIRS or (not wide and d % 64 != 0)):
        return "prod"
    return "wide" if wide else "two"


def gemm_height(m, n, nb=1):
    """launch_gemm's score: W / (ceil(W / 256) 256) x {0.95, 1.0, 0.966}[height] x min(1, (W / 512)^0.22); ties go to the taller tile"""
    best, best_score = 0, -1.0
    for h, worth in ((32, 0.95), (64, 1.0), (128, 0.966)):
        w = ((n + 63) // 64) * ((m + h - 1) // h) * nb
        score = w / ((w + 255) // 256 * 256) * worth * ((w / 512.0) ** 0.22 if w < 512 else 1.0)
        if score >= best_score:
            best, best_score = h, score
    return best


def gemm_form(m, n, k, lda, ldb, nb=1, aligned=True, mid=False, seg=False):
    """the counter of vgpa_ld_launch_counts a stage product advances (launch_gemm, launch_gemm_bm)"""
    h = gemm_height(m, n, nb)
    full = m % h == 0 and n % 64 == 0 and k % 16 == 0
    vec = full and lda % 2 == 0 and ldb % 2 == 0 and aligned
    if vec and seg and not mid:
        form = "seg4" if (k // 16) % 4 == 0 else "seg"
    elif vec and not seg:
        form = "vec4" if not mid and (k // 16) % 4 == 0 else "vec"
    else:
        form = "full" if full else "checked"
    return f"gemm{h}_{form}"


# --------------------------------------------------------------------------- #
#  Operator level
# --------------------------------------------------------------------------- #
# path, D, problems, flag name, VGPA_STAGE_FUSED, VGPA_STAGE_WIDE, non-symmetric inputs, virtual ranks, sub-blocks (None: the default schedule)
LdUnit = collections.namedtuple("LdUnit", "path d batch flag fused_env wide_env nonsym world chunks")
LdOp = collections.namedtuple("LdOp", LdUnit._fields + ("method", "regime"))


def _u(path, d, batch=1, flag=None, fused_env=None, wide_env=None, nonsym=False, world=1, chunks=None):
    return LdUnit(path, d, batch, flag, fused_env, wide_env, nonsym, world, chunks)


LD_UNITS = (
    # k_stage_prod by the default rule: a 1-row last tile and a k tail of 1; 15 and 15; odd D with four tiles; a batch
    [_u("prod", 65), _u("prod", 79), _u("prod", 97), _u("prod", 96, 3)] +
    # k_stage_wide by the default rule: 17 tiles, three macro-rows, above kStageProdMaxD (first: Euler and Heun by the rotation); 11 tiles,
    # two macro-rows, an odd diagonal count, 66 pairs; 8 x 10 pairs; 9 tiles, a second macro-row of one row, a 2-row last tile
    [_u("wide", 514), _u("wide", 330), _u("wide", 128, 8), _u("wide", 258, 2)] +
    [_u("wide_forced", 72, fused_env="0"), _u("wide_forced", 130, fused_env="0")] +
    # the two-kernel stage by the default rule: k_gemm_v with four register sets on 32-row tiles, k_stage_sym with 78 pairs
    [_u("two", 384)] +
    # ... forced: vec4; the bounds-checked product with a ragged k_stage_sym; a batch
    [_u("two_forced", 128, fused_env="0", wide_env="0"), _u("two_forced", 130, fused_env="0", wide_env="0"),
     _u("two_forced", 96, 3, fused_env="0", wide_env="0")] +
    # the literal non-symmetric path: checked product + k_transpose + k_stage; the 16-byte product; a batch
    [_u("nonsym", 80, nonsym=True), _u("nonsym", 128, nonsym=True), _u("nonsym", 96, 3, nonsym=True)] +
    [_u("library", 96, flag="FLAG_LIBRARY_GEMM")] +
    # the row-sharded native driver on virtual ranks: the default 4 sub-blocks; three ranks (2 sub-blocks of the checked kernel); serial
    [_u("sharded", 128, world=2), _u("sharded", 96, world=3), _u("sharded", 128, world=2, chunks=0)])
LD_PATHS = tuple(dict.fromkeys(u.path for u in LD_UNITS))
SHARDED_DEFAULT_CHUNKS = {(128, 2): 4, (96, 3): 2}           # (what test_native_sharded_driver_with_virtual_ranks asserts of the library)


def _ld_ops():
    """units x methods x regimes thinned as test_stepper_rounding_cpu._op_cases thins them -- unit i of a path runs method (i + r) mod 4 in
    regime r -- with as many further shifts as the path needs for every (path, method, regime) to occur: none from four units on, one
    (+2) at two or three units, all four methods at one unit."""
    cases = []
    for path in LD_PATHS:
        units = [u for u in LD_UNITS if u.path == path]
        shifts = (0,) if len(units) >= 4 else (0, 2) if len(units) >= 2 else (0, 1, 2, 3)
        for i, u in enumerate(units):
            for r, regime in enumerate(OP_REGIMES):
                for shift in shifts:
                    cases.append(LdOp(*u, METHODS[(i + r + shift) % 4], regime))
    return cases


LD_OPS = _ld_ops()


def ld_id(c):
    return "-".join(f"{k}{v}" if k in ("world", "chunks", "batch") else str(v)
                    for k, v in zip(c._fields, c) if v is not None and v is not False and not (k in ("batch", "world") and v == 1)
                    and k not in ("fused_env", "wide_env"))


def ref_case(c):
    """the case of test_stepper_rounding_cpu whose inputs and reference this one runs: they depend on (D, n_pts, method, regime, symmetry)
    and the problem number only, so the paths that run the same unit share one reference (op_reference is keyed by the case)"""
    return OpCase("large_d", c.d, c.batch, None, None, c.nonsym, N_PTS, c.method, c.regime)


def ld_op_reference(c, k):
    return op_reference(ref_case(c), k)


def expected_launches(c, n_pts=N_PTS):
    """The counters of vgpa_ld_launch_counts that one forward and one backward recursion of the case advance, and how far (every other
    counter stays): a step issues its stages one by one, the mid-point operand once per step where a stage reads it."""
    tot, mid = STAGES[c.method]
    steps = (n_pts - 1) * 2
    d, nb = c.d, c.batch
    path = {"wide_forced": "wide", "two_forced": "two"}.get(c.path, c.path)
    once = {"mid": steps} if mid else {}
    if path in ("prod", "wide", "two"):
        assert stage_path(d, nb, c.fused_env, c.wide_env) == path, (c, stage_path(d, nb, c.fused_env, c.wide_env))
    if path == "prod":
        per = (n_pts - 1)
        out = {"stage_prod_fwd": per * (tot - mid), "stage_prod_fwd_mid": per * mid, "stage_prod_bwd": per * (tot - mid),
               "stage_prod_bwd_mid": per * mid}
    elif path == "wide":
        out = dict(once, stage_wide_fwd=(n_pts - 1) * tot, stage_wide_bwd=(n_pts - 1) * tot)
    elif path == "two":
        out = dict(once, stage_sym=steps * tot)
        out[gemm_form(d, d, d, d, d, nb)] = steps * tot
    elif path == "nonsym":
        assert stage_path(d, nb, literal=True) == "two"
        out = dict(once, transpose=steps * tot, stage_rows=steps * tot)
        out[gemm_form(d, d, d, d, d, nb)] = 2 * steps * tot
    elif path == "library":
        assert stage_path(d, nb, library=True) == "two" and nb == 1
        out = dict(once, library_gemm=steps * tot, stage_sym=steps * tot)
    elif path == "sharded":
        mp = d // c.world
        chunks = SHARDED_DEFAULT_CHUNKS[(d, c.world)] if c.chunks is None else c.chunks
        out = {"stage_rows": steps * tot * c.world}
        if mid:
            out["mid_cols"] = steps * c.world
        if chunks:
            sub = mp // chunks
            out[gemm_form(mp, d, c.world * sub, d, d, seg=True)] = steps * tot * chunks * c.world
        else:
            out[gemm_form(mp, d, d, d, d)] = steps * tot * c.world
    return {k: v for k, v in out.items() if v}


LD_OP_REFS = list(dict.fromkeys(ref_case(c) for c in LD_OPS))


@pytest.mark.parametrize("c", LD_OP_REFS, ids=case_id)
def test_large_d_operator_case_is_in_its_regime_and_the_reference_holds(c):
    """test_stepper_rounding_cpu's own function on every distinct input set of LD_OPS: the same assertions, nothing restated."""
    base.test_operator_case_is_in_its_regime_and_the_reference_holds(c)


def test_large_d_operator_table_meets_the_coverage_conditions():
    """Every (path, method, regime) occurs, every unit runs in both regimes, D = 514 runs Euler and Heun only; every case's path follows from
    run_stage's rule and its counters from launch_gemm's (expected_launches asserts the first and applies the second)."""
    assert {(c.path, c.method, c.regime) for c in LD_OPS} == {(p, m, r) for p in LD_PATHS for m in METHODS for r in OP_REGIMES}
    for u in LD_UNITS:
        assert {c.regime for c in LD_OPS if c[:len(u)] == u} == set(OP_REGIMES), u
    assert {c.method for c in LD_OPS if c.d == 514} == {"euler", "heun"}
    assert len(LD_OPS) == len(set(LD_OPS)) and len({ld_id(c) for c in LD_OPS}) == len(LD_OPS)
    moved = set()
    for c in LD_OPS:
        want = expected_launches(c)
        assert want and set(want) <= set(_lib.LD_COUNT_NAMES), (c, want)
        moved |= set(want)
    assert stage_path(258) == "prod" and stage_path(258, 2) == "wide" and stage_path(330) == "wide" and stage_path(128, 8) == "wide"
    assert stage_path(384) == "two" and stage_path(514) == "wide" and stage_path(97) == "prod" and stage_path(96, 3) == "prod"
    by_path = {p: set().union(*(set(expected_launches(c)) for c in LD_OPS if c.path == p)) for p in LD_PATHS}
    assert by_path["prod"] == {"stage_prod_fwd", "stage_prod_fwd_mid", "stage_prod_bwd", "stage_prod_bwd_mid"}
    assert by_path["wide"] == by_path["wide_forced"] == {"stage_wide_fwd", "stage_wide_bwd", "mid"}
    assert by_path["two"] == {"gemm32_vec4", "stage_sym", "mid"}
    assert by_path["two_forced"] == {"gemm32_vec4", "gemm32_checked", "stage_sym", "mid"}
    assert by_path["nonsym"] == {"gemm32_vec4", "gemm32_checked", "transpose", "stage_rows", "mid"}
    assert by_path["library"] == {"library_gemm", "stage_sym", "mid"}
    assert by_path["sharded"] == {"gemm32_seg", "gemm64_checked", "gemm32_vec4", "stage_rows", "mid_cols"}
    print("counters the operator level advances:", sorted(moved))


# --------------------------------------------------------------------------- #
#  Fused level (Lorenz-96): Context.sweep / fetch / energy_parts
# --------------------------------------------------------------------------- #
# path, D, Np, problems, flag name, VGPA_STAGE_FUSED, VGPA_STAGE_WIDE, Sigma form; near the optimum (RK4) and stiff (the methods rotate)
LdFusedUnit = collections.namedtuple("LdFusedUnit", "path d n_pts batch flag fused_env wide_env sigma method")
LD_FUSED_UNITS = (
    LdFusedUnit("prod", 130, 6, 1, None, None, None, "diag", None),
    LdFusedUnit("wide_forced", 130, 6, 1, None, "0", None, "diag", None),
    LdFusedUnit("two_forced", 130, 6, 1, None, "0", "0", "diag", None),
    LdFusedUnit("dense_sigma", 128, 5, 1, None, None, None, "dense", None),
    LdFusedUnit("batched", 96, 5, 4, None, None, None, "diag", "heun"),
    LdFusedUnit("prod200", 200, 4, 1, None, None, None, "diag", None),
    LdFusedUnit("library", 96, 9, 1, "FLAG_LIBRARY_GEMM", None, None, "diag", None),
    LdFusedUnit("library_streamed", 96, 9, 1, "FLAG_LIBRARY_GEMM|FLAG_STREAM_LARGE_D", None, None, "diag", None))
LdFused = collections.namedtuple("LdFused", LdFusedUnit._fields + ("regime",))
# (the three stage versions of D = 130 run the same method: they share x* and the references; the library pair likewise)
_ROT = {"prod": 0, "wide_forced": 0, "two_forced": 0, "dense_sigma": 1, "prod200": 2, "library": 3, "library_streamed": 3}
LD_FUSED = [LdFused(*u[:-1], u.method or ("rk4" if regime == "near" else METHODS[(_ROT[u.path] + 3) % 4]), regime)
            for u in LD_FUSED_UNITS for regime in ("near", "stiff")]


def fused_ref_case(c):
    """the FusedCase whose problem, x and reference this case runs (test_stepper_rounding_cpu keys them by the whole case)"""
    return FusedCase("large_d", "L96", c.d, c.n_pts, c.method, c.batch, None, c.sigma, c.regime)


def fused_expected_launches(c):
    """one forward and one backward recursion inside the sweep: the operator level's rule on the sweep's grid"""
    path = {"dense_sigma": "prod", "batched": "prod", "prod200": "prod", "library_streamed": "library"}.get(c.path, c.path)
    op = LdOp(path, c.d, c.batch, None, c.fused_env, c.wide_env, False, 1, None, c.method, c.regime)
    return expected_launches(op, n_pts=c.n_pts)


LD_FUSED_REFS = list(dict.fromkeys(fused_ref_case(c) for c in LD_FUSED))


@pytest.mark.parametrize("c", LD_FUSED_REFS, ids=case_id)
def test_large_d_fused_case_is_in_its_regime_and_the_reference_holds(c):
    """test_stepper_rounding_cpu's own function on every distinct (problem, x) of LD_FUSED."""
    base.test_fused_case_is_in_its_regime_and_the_reference_holds(c)


def test_large_d_fused_table_meets_the_coverage_conditions():
    assert {(c.path, c.regime) for c in LD_FUSED} == {(u.path, r) for u in LD_FUSED_UNITS for r in ("near", "stiff")}
    assert {c.method for c in LD_FUSED if c.regime == "stiff"} == set(METHODS)
    assert {c.method for c in LD_FUSED if c.path == "batched"} == {"heun"}
    assert len({fused_ref_case(c) for c in LD_FUSED if c.d == 130}) == 2          # three stage versions, one x* and one stiff x
    for c in LD_FUSED:
        assert fused_expected_launches(c), c
    assert [(u.d, u.n_pts, u.batch) for u in LD_FUSED_UNITS] == [(130, 6, 1)] * 3 + [(128, 5, 1), (96, 5, 4), (200, 4, 1), (96, 9, 1), (96, 9, 1)]


# --------------------------------------------------------------------------- #
#  The bound still discriminates at these sizes
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("regime", OP_REGIMES)
@pytest.mark.parametrize("d", [130, 330])
def test_a_scaled_slope_is_caught_above_64(d, regime):
    """test_stepper_rounding_cpu._mutant_rk4 (fourth slope of S_t forward and of Psi_t backward times 1 + 2^-30) at D = 130 and D = 330:
    it passes rel_err < 1e-9 against the oracle in every quantity and misses the bound in S_t and in Psi_t; with eps = 0 the same code
    IS the oracle.  err_o grows with the length of the sums, so this is where the bound could have stopped discriminating."""
    c = OpCase("large_d", d, 1, None, None, False, N_PTS, "rk4", regime)
    ext, orc = op_reference(c, 0)
    same = base._mutant_rk4(c, 0, eps=0.0)
    assert all(np.array_equal(same[q], orc[q]) for q in OP_QUANTITIES)
    got = base._mutant_rk4(c, 0)
    for q in OP_QUANTITIES:
        old, err_o, err_k = rel_err(got[q], orc[q]), ld_rel_err(orc[q], ext[q]), ld_rel_err(got[q], ext[q])
        print(f"[mutant D={d} {regime}] {q}: against the oracle {old:.2e}; err_o={err_o:.2e} err_k={err_k:.2e} "
              f"ratio={ratio(err_k, err_o):.3g} (margin over FACTOR: {ratio(err_k, err_o) / FACTOR:.3g})")
        assert old < 1e-9
        assert (err_k <= bound(err_o)) == (q in ("mt", "lamt")), q


# --------------------------------------------------------------------------- #
#  Exact stage products: integer operands, every partial sum representable
# --------------------------------------------------------------------------- #
EXACT_MAX = 2 ** 10                     # |a|, |b| <= 2^10, integers; the mid-point form averages two such a's: half-integers
EXACT_K_MAX = 4096


def exact_operand(rng, shape):
    """integer-valued fp64 entries in [-2^10, 2^10]"""
    return rng.integers(-EXACT_MAX, EXACT_MAX + 1, size=shape).astype(np.float64)


# name -> (M, N, K, mid, lda parity (0 even, 1 odd), pointers 16-byte aligned, counter).  The K-chunk launches are in SEG_CASES.
GemmCase = collections.namedtuple("GemmCase", "name m n k mid odd_lda aligned counter")
GEMM_CASES = (
    GemmCase("32-checked", 100, 130, 72, False, 1, False, "gemm32_checked"),
    GemmCase("32-full", 128, 128, 64, False, 1, True, "gemm32_full"),
    GemmCase("32-full-unaligned", 128, 128, 64, False, 0, False, "gemm32_full"),
    GemmCase("32-vec", 128, 128, 48, False, 0, True, "gemm32_vec"),
    GemmCase("32-vec4", 128, 128, 64, False, 0, True, "gemm32_vec4"),
    GemmCase("32-mid-checked", 96, 160, 40, True, 0, True, "gemm32_checked"),
    GemmCase("32-mid-vec", 128, 128, 48, True, 0, True, "gemm32_vec"),
    GemmCase("32-mid-vec-k64", 128, 128, 64, True, 0, True, "gemm32_vec"),           # (the four-set loop has no mid-point form)
    GemmCase("32-mid-full", 128, 128, 64, True, 1, True, "gemm32_full"),
    GemmCase("64-checked", 32, 64, 40, False, 0, True, "gemm64_checked"),
    GemmCase("64-full", 2048, 2048, 64, False, 1, True, "gemm64_full"),
    GemmCase("64-vec", 2048, 2048, 48, False, 0, True, "gemm64_vec"),
    GemmCase("64-vec4", 2048, 2048, 64, False, 0, True, "gemm64_vec4"),
    GemmCase("64-vec4-shard-block", 512, 4096, 128, False, 0, True, "gemm64_vec4"),
    GemmCase("128-checked", 928, 3968, 48, False, 0, True, "gemm128_checked"))
# name -> (M, N, ranks, sub-blocks, rows of a rank's block of the operand): launch j multiplies sub-block j of every rank's block
# (seg_tiles = sub / 16 out of every mp k), K = ranks x mp in all; `chunk` the counter of the chunk launches, `whole` of ONE segmented
# launch over every k in natural order
SegCase = collections.namedtuple("SegCase", "name m n world chunks mp chunk whole")
SEG_CASES = (
    SegCase("32-seg", 64, 128, 2, 4, 64, "gemm32_seg", "gemm32_seg4"),
    SegCase("64-checked-seg", 32, 96, 3, 2, 32, "gemm64_checked", "gemm64_checked"),
    SegCase("32-seg4", 64, 256, 2, 2, 128, "gemm32_seg4", "gemm32_seg4"),
    SegCase("64-seg", 512, 4096, 2, 2, 32, "gemm64_seg", "gemm64_seg4"),
    SegCase("64-seg4", 512, 4096, 1, 2, 128, "gemm64_seg4", "gemm64_seg4"))
# what launch_gemm cannot reach (rounding section): at M a multiple of 128 the 64-row tile has twice the workgroups, so its
# balance and its (W / 512)^0.22 are no smaller and its worth is 1.0 against 0.966 -- the 128-row tile wins at ragged M only
UNREACHABLE = ("gemm128_full", "gemm128_vec", "gemm128_vec4", "gemm128_seg", "gemm128_seg4")


def test_exact_products_are_exact_and_the_shapes_select_their_kernels():
    """K 2^20 < 2^53 (2^21 in units of the half-integers' 1/2) for the largest K: every product and partial sum of the integer operands is
    representable, in any order of summation.  numpy's fp64 dot equals the int64 product at the smallest shape.  Every shape selects,
    by launch_gemm's restated score, the tile height and form its name says; the tables reach every counter that can be reached."""
    assert EXACT_K_MAX * EXACT_MAX ** 2 < 2 ** 53 and 2 * EXACT_K_MAX * (2 * EXACT_MAX) * EXACT_MAX < 2 ** 53
    assert all(c.k <= EXACT_K_MAX for c in GEMM_CASES) and all(c.world * c.mp <= EXACT_K_MAX for c in SEG_CASES)
    rng = np.random.default_rng(1)
    small = min(GEMM_CASES, key=lambda c: c.m * c.n * c.k)
    a, a1, b = exact_operand(rng, (small.m, small.k)), exact_operand(rng, (small.m, small.k)), exact_operand(rng, (small.k, small.n))
    assert np.max(np.abs(a)) <= EXACT_MAX and np.array_equal(a, np.rint(a))
    want = a.astype(np.int64).dot(b.astype(np.int64))
    assert np.array_equal(a.dot(b), want.astype(np.float64)) and np.array_equal(want.astype(np.float64).astype(np.int64), want)
    twice = (a.astype(np.int64) + a1.astype(np.int64)).dot(b.astype(np.int64))         # the mid-point form, in units of 1/2
    assert np.array_equal((0.5 * (a + a1)).dot(b) * 2.0, twice.astype(np.float64))
    for c in GEMM_CASES:
        lda = c.k + 2 + c.odd_lda                          # (NN; the transposed operand has M in place of K: the parity is the same)
        assert gemm_form(c.m, c.n, c.k, lda, c.n + 2, aligned=c.aligned, mid=c.mid) == c.counter, c
        assert gemm_form(c.m, c.n, c.k, c.m + 2 + c.odd_lda, c.n + 2, aligned=c.aligned, mid=c.mid) == c.counter, c
    for c in SEG_CASES:
        sub = c.mp // c.chunks
        assert sub % 16 == 0 and c.mp % c.chunks == 0
        assert gemm_form(c.m, c.n, c.world * sub, 2, 2, seg=True) == c.chunk, c
        assert gemm_form(c.m, c.n, c.world * c.mp, 2, 2, seg=True) == c.whole, c
    reached = {c.counter for c in GEMM_CASES} | {c.chunk for c in SEG_CASES} | {c.whole for c in SEG_CASES}
    gemm = {n for n in _lib.LD_COUNT_NAMES if n.startswith("gemm")}
    assert gemm - reached == set(UNREACHABLE), sorted(gemm - reached)
    # the argument for UNREACHABLE, checked over every launch a recursion up to D = 8192 or a row block of it can issue
    for m in range(128, 8192 + 1, 128):
        for n in (64, 128, 192, 256, 384, 512, 1024, 2048, 3968, 4096, 8192):
            for nb in (1, 3, 8):
                assert gemm_height(m, n, nb) != 128, (m, n, nb)
    assert gemm_height(928, 3968) == 128


def test_launch_counter_names_agree_with_the_header():
    """_lib.LD_COUNT_NAMES in the order of include/vgpa_hip.h's VGPA_LD_COUNT_* / VGPA_LD_GEMM_*; the library reports as many."""
    import os
    import re
    from conftest import ROOT
    from vgpa_amd import large_d
    header = open(os.path.join(ROOT, "include", "vgpa_hip.h")).read()
    enums = {k: int(v) for k, v in re.findall(r"\b(VGPA_LD_[A-Z0-9_]+)\s*=\s*(-?\d+)", header)}
    n, first = enums.pop("VGPA_LD_COUNT_N"), enums.pop("VGPA_LD_COUNT_GEMM")
    forms = {k[len("VGPA_LD_GEMM_"):].lower(): v for k, v in enums.items() if k.startswith("VGPA_LD_GEMM_")}
    plain = {k[len("VGPA_LD_COUNT_"):].lower(): v for k, v in enums.items() if k.startswith("VGPA_LD_COUNT_")}
    assert forms == {f: i for i, f in enumerate(_lib.LD_GEMM_FORMS)}
    want = dict(plain)
    for hi, h in enumerate((32, 64, 128)):
        for f, i in forms.items():
            want[f"gemm{h}_{f}"] = first + 6 * hi + i
    assert want == {name: i for i, name in enumerate(_lib.LD_COUNT_NAMES)} and n == len(_lib.LD_COUNT_NAMES)
    counts = large_d.launch_counts()                       # (host-side table: readable without a device)
    assert list(counts) == list(_lib.LD_COUNT_NAMES) and all(isinstance(v, int) and v >= 0 for v in counts.values())
    assert large_d.launched(counts, counts) == {}
