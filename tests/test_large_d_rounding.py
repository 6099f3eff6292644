"""
GPU suite (-m gpu): every implementation of a Runge-Kutta stage above D = 64 -- k_stage_prod, k_stage_wide, the two-kernel stage (k_mid,
k_gemm / k_gemm_v, k_stage_sym), the literal non-symmetric path (k_transpose, a second product, k_stage), the batched drivers,
VGPA_FLAG_LIBRARY_GEMM, the row-sharded native driver, the fused sweep above D = 72 -- held to ROUNDING ERROR against the longdouble
restatement of the sweep (tests/extended_ref.py), and every instantiation of the stage product that launch_gemm can reach held to the
EXACT fp64 product on integer operands.  Cases, inputs, references and expected launches come from test_large_d_rounding_cpu.py, which
asserts their regimes without a device.

The bound, per case, compared problem and quantity q (test_stepper_rounding.py's, FACTOR = 32 unchanged):

    err_k(q) <= FACTOR * max(err_o(q), 2^-53)

Before a number, every case asserts plan()["fwd"] == plan()["bwd"] == "large_d" and, by difference of vgpa_ld_launch_counts around the
call, that exactly the kernels it names ran, as often as its recursion has stages, and no other stage kernel or product did.

Measured on an MI355X (profiles/large_d_rounding_gputests.log has every compared problem; err_o is computed on the host of the same run).
No kernel of the parent commit exceeded its bound, every counter assertion held, and every exact product was bit-equal with its sentinel
bands intact.  Worst ratio err_k / max(err_o, 2^-53) per path, with the quantity that gave it:
  operator level   k_stage_prod 1.29 (m_t), k_stage_wide by the default rule 1.41 (S_t) and forced 1.39 (m_t), the two-kernel stage by the
                   default rule 1.37 (m_t) and forced 1.22 (m_t), literal non-symmetric 1.52 (m_t), library product 1.09 (m_t), row-sharded
                   native driver 1.28 (Psi_t; S_t 1.26)
  fused level      D = 130 on k_stage_prod, k_stage_wide and the two-kernel stage alike -- the three agree bit for bit -- 3.22 (E_sde;
                   dEsde_dm 3.13, dEsde_dS 2.36, lam_t 2.20, gLa 2.07, Psi_t 2.03, gLb 2.00); dense Sigma D = 128 2.16 (lam_t; gLb 1.93,
                   dEsde_dm 1.85); four problems D = 96 Heun 2.79 (gLb and lam_t; dEsde_dm 2.59); D = 200 3.62 (gLb; lam_t 3.61, dEsde_dm
                   3.17, gLa 2.94, Psi_t 2.52); library product D = 96 resident and time-chunked alike 3.24 (lam_t; gLb 2.77, dEsde_dm 2.61)
Worst ratio per quantity:
  operator level   m_t 1.52, S_t 1.41, lam_t 1.25, Psi_t 1.40
  fused level      F 0.72, gLa 2.94, gLb 3.62, E_sde 3.22, E_obs 1.00, m_t 1.03, S_t 1.01, lam_t 3.61, Psi_t 2.52, dEsde_dm 3.17, dEsde_dS 2.36
The module takes 93 s, 133 cases; the slowest are the longdouble references on the host (D = 514 Heun 7.8 s, D = 384 RK4 6.3 s, the
60 SCG iterations of D = 200 7.7 s), no kernel takes a second.
"""
import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.large_d import launch_counts, launched
from test_gpu_edge_cases import gpu_context
from test_large_d import _run_native_virtual_ranks
from test_large_d_rounding_cpu import (GEMM_CASES, LD_FUSED, LD_OPS, N_PTS, SEG_CASES, SHARDED_DEFAULT_CHUNKS, UNREACHABLE, exact_operand,
                                       expected_launches, fused_expected_launches, fused_ref_case, ld_id, ld_op_reference, ref_case)
from test_stepper_rounding import FETCHED, MATRIX_KEYS, STREAM_CHUNK, STREAMED_QUANTITIES, psi_recovery_term
from test_stepper_rounding_cpu import (DT, FUSED_QUANTITIES, OP_QUANTITIES, bound, checked, fused_problem, fused_reference, fused_x, ld_rel_err,
                                       op_problem, op_shared, ratio)

pytestmark = pytest.mark.gpu
WORST = {}                 # (path, quantity) -> the worst ratio err_k / max(err_o, 2^-53) of this process's run
RAN = set()                # the cases of this module that ran in this process (test_worst_ratios_of_the_module)


def _flags(names):
    return sum(getattr(_lib, n) for n in names.split("|")) if names else 0


def _stage_version(monkeypatch, c):
    """the only environment the module sets: which implementation of the stage run_stage may take (read per call)"""
    if c.fused_env is not None:
        monkeypatch.setenv("VGPA_STAGE_FUSED", c.fused_env)
    if c.wide_env is not None:
        monkeypatch.setenv("VGPA_STAGE_WIDE", c.wide_env)


def compare(tag, path, got, ext, orc, names, extra=None):
    """One line per compared problem: for every quantity  name err_o/err_k/ratio  (ratio = err_k / max(err_o, 2^-53)).  The quantities
    over their bound are returned."""
    fails, line = [], []
    for q in names:
        err_o, err_k = ld_rel_err(orc[q], ext[q]), ld_rel_err(np.reshape(got[q], np.shape(ext[q])), ext[q])
        more = (extra or {}).get(q, 0.0)
        rat = ratio(err_k, err_o)
        line.append(f"{q} {err_o:.1e}/{err_k:.1e}/{rat:.2f}" + (f"+{more:.1e}" if more else ""))
        WORST[(path, q)] = max(WORST.get((path, q), 0.0), rat)
        if not err_k <= bound(err_o, more):
            fails.append((tag, q, err_o, err_k, bound(err_o, more)))
    print(tag, " ".join(line))
    return fails


# ---- a. the stage paths, operator level -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in LD_OPS if c.path != "sharded"], ids=ld_id)
def test_stage_paths_operator_level(c, monkeypatch):
    """Context("NONE").solve_fwd / solve_bwd above D = 64, benign and stiff, on the path the case names: every problem of the context has
    its own A_t; the first and the last are compared in m_t, S_t, lam_t and Psi_t."""
    _stage_version(monkeypatch, c)
    rc, batch = ref_case(c), c.batch
    m0, s0, sigma = op_shared(rc)
    a, b, gm, gs, jm, js = (np.stack(v) for v in zip(*(op_problem(rc, k) for k in range(batch))))
    ctx = va.Context("NONE", c.method, c.d, N_PTS, DT, sigma=sigma, batch=batch, flags=_flags(c.flag))
    plan = ctx.plan()
    assert plan["fwd"] == plan["bwd"] == "large_d", plan
    before = launch_counts()
    mt, st = ctx.solve_fwd(a, b, m0, s0, sigma)
    lam, psi = ctx.solve_bwd(a, gm, gs, jm, js)
    ran = launched(before)
    ctx.close()
    assert ran == expected_launches(c), (ran, expected_launches(c))
    got = {q: np.reshape(v, (batch,) + v.shape[-(2 + (q in MATRIX_KEYS)):]) for q, v in zip(OP_QUANTITIES, (mt, st, lam, psi))}
    fails = []
    for k in checked(batch):
        ext, orc = ld_op_reference(c, k)
        fails += compare(f"[op {ld_id(c)}] k={k}", c.path, {q: got[q][k] for q in OP_QUANTITIES}, ext, orc, OP_QUANTITIES)
    RAN.add(c)
    assert not fails, fails


@pytest.mark.parametrize("c", [c for c in LD_OPS if c.path == "sharded"], ids=ld_id)
def test_row_sharded_native_driver(c):
    """vgpa_shard_solve_fwd / _bwd on virtual ranks (k_stage with Mp < D; the K-chunk launches of the pipelined schedule, or one product
    per stage on the serial one; k_mid_cols): the owners' time slices tile the grid, and every owner's slice is held to the bound --
    in the norm of the whole quantity, as everywhere (the last grid point alone has lam_t = Psi_t = 0)."""
    rc = ref_case(c)
    (m0, s0, sigma), (a, b, gm, gs, jm, js) = op_shared(rc), op_problem(rc, 0)
    before = launch_counts()
    used, ranks = _run_native_virtual_ranks(c.method, c.d, N_PTS, c.world, chunks=c.chunks, inputs=(a, b, m0, s0, sigma, gm, gs, jm, js))
    ran = launched(before)
    assert used == (SHARDED_DEFAULT_CHUNKS[(c.d, c.world)] if c.chunks is None else c.chunks)
    assert ran == expected_launches(c), (ran, expected_launches(c))
    ext, orc = ld_op_reference(c, 0)
    got = {q: np.full(np.shape(ext[q]), np.nan) for q in OP_QUANTITIES}
    for r in ranks:
        lo, hi = r["slice"]
        for q in OP_QUANTITIES:
            assert r[q].shape == got[q][lo:hi].shape, (q, r[q].shape)
            got[q][lo:hi] = r[q]
    assert all(np.all(np.isfinite(v)) for v in got.values())
    fails = compare(f"[op {ld_id(c)}] ranks={[r['slice'] for r in ranks]}", c.path, got, ext, orc, OP_QUANTITIES)
    RAN.add(c)
    assert not fails, fails


# ---- a. the stage paths, fused level --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", LD_FUSED, ids=lambda c: "-".join(str(v) for v in (c.path, c.d, c.n_pts, c.batch, c.method, c.regime)))
def test_fused_sweep_above_72(c, monkeypatch):
    """Lorenz-96, Context.sweep / fetch / energy_parts near the optimum and on stiff A_t: D = 130 on all three stage versions, a dense
    Sigma (D = 128: the dense-Sigma gradient kernels), four problems (D = 96, Heun), ragged tiles (D = 200), VGPA_FLAG_LIBRARY_GEMM
    resident and time-chunked (what the chunked sweep still keeps is compared)."""
    _stage_version(monkeypatch, c)
    rc = fused_ref_case(c)
    p, _ = fused_problem("L96", c.d, c.n_pts, c.method, c.sigma)
    n, d, batch, streamed = c.n_pts, c.d, c.batch, c.path == "library_streamed"
    names = STREAMED_QUANTITIES if streamed else FUSED_QUANTITIES
    ctx = gpu_context(p, batch=batch, flags=_flags(c.flag))
    plan = ctx.plan()
    assert plan["fwd"] == plan["bwd"] == "large_d", plan
    if streamed:
        ctx.set_option(_lib.OPT_LD_CHUNK, STREAM_CHUNK)
    xb = np.stack([fused_x(rc, k) for k in range(batch)])
    before = launch_counts()
    f, g = ctx.sweep(xb if batch > 1 else xb[0])
    ran = launched(before)
    assert ctx.streaming == streamed and ctx.resident()["cached"]
    got = dict(F=np.atleast_1d(f), g=np.reshape(g, (batch, -1)))
    for q in [q for q in FETCHED if q in names]:
        got[q] = np.reshape(ctx.fetch(q), (batch, n) + ((d, d) if q in MATRIX_KEYS else (d,)))
    _, es, eo = ctx.energy_parts()
    got["Esde"], got["Eobs"] = np.atleast_1d(es), np.atleast_1d(eo)
    after = launched(before)
    ctx.close()
    want = fused_expected_launches(c)
    if streamed:           # (the chunked sweep runs the forward recursion again per chunk: the same kernels, at least as often)
        assert set(ran) == set(want) and all(ran[k] >= want[k] for k in want), (ran, want)
    else:
        assert ran == want and after == ran, (ran, after, want)
    fails, k_a = [], n * d * d
    for k in checked(batch):
        ext, orc = fused_reference(rc, k)
        mine = {q: got[q][k] for q in names if q not in ("gLa", "gLb")}
        mine["gLa"], mine["gLb"] = got["g"][k][:k_a], got["g"][k][k_a:]
        extra = {"psit": psi_recovery_term(p, fused_x(rc, k), ext["psit"])} if plan["store_q"] and "psit" in names else None
        fails += compare(f"[fused {c.path}-{d}-{c.method}-{c.regime}] k={k}", "fused " + c.path, mine, ext, orc, names, extra)
    RAN.add(c)
    assert not fails, fails


# ---- b. the stage product, exactly ----------------------------------------------------------------------------------------------
BAND, SENTINEL = 64, -7.0


def _view(values, ld, off):
    """a host buffer of NaN with `values` (rows x cols) as the view [rows][ld] starting `off` doubles in; two rows of NaN behind it"""
    rows, cols = values.shape
    assert ld >= cols
    buf = np.full(off + (rows + 2) * ld, np.nan)
    buf[off:off + rows * ld].reshape(rows, ld)[:, :cols] = values
    return buf


def _unpack(c_host, m, n, cw):
    """the column-chunk packed C[(j / cw) M cw + i cw + (j % cw)] between its two sentinel bands -> (M, N)"""
    assert np.all(c_host[:BAND] == SENTINEL) and np.all(c_host[BAND + m * n:] == SENTINEL), "a sentinel band was written"
    inner = c_host[BAND:BAND + m * n]
    assert not np.any(np.isnan(inner)), f"{int(np.sum(np.isnan(inner)))} elements of C were never written"
    return inner.reshape(n // cw, m, cw).transpose(1, 0, 2).reshape(m, n)


def _small_cw(n):
    return next(w for w in (64, 32, 26, 16) if n % w == 0 and w < n)


def _c_buffer(m, n, dev):
    import torch
    c = torch.full((2 * BAND + m * n,), float("nan"), dtype=torch.float64, device=dev)
    c[:BAND] = SENTINEL
    c[BAND + m * n:] = SENTINEL
    return c


@pytest.mark.parametrize("transa", [False, True], ids=["nn", "tn"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: c.name)
def test_stage_product_is_exact(case, transa):
    """vgpa_ld_gemm on integer operands (|a|, |b| <= 2^10; the mid-point form averages two: half-integers): every partial sum is
    representable, so C must equal numpy's fp64 product bit for bit whatever the order of summation.  The operands are views into larger
    buffers of NaN with leading dimensions above the minimum; C is NaN between two sentinel bands; cw = N and a cw dividing N."""
    import torch
    from legacy_sharded import HipStageBackend
    be = HipStageBackend()
    lib, st, dev = be._lib, be._stream(), torch.device("cuda", 0)
    m, n, k = case.m, case.n, case.k
    rng = np.random.default_rng([m, n, k, int(transa), int(case.mid)])
    shape = (k, m) if transa else (m, k)
    a0, a1, b = exact_operand(rng, shape), (exact_operand(rng, shape) if case.mid else None), exact_operand(rng, (k, n))
    lda, ldb = shape[1] + 2 + case.odd_lda, n + 2
    off = 2 * lda + (2 if case.aligned else 1) - (2 * lda) % 2           # even where the pointers are to be 16-byte aligned, else odd
    assert (off % 2 == 0) == case.aligned
    a0_d = torch.as_tensor(_view(a0, lda, off), device=dev)
    a1_d = torch.as_tensor(_view(a1, lda, off), device=dev) if case.mid else None
    b_off = off - (2 * lda - (2 * lda) % 2) + 2 * ldb
    b_d = torch.as_tensor(_view(b, ldb, b_off), device=dev)
    assert a0_d.data_ptr() % 16 == 0 and b_d.data_ptr() % 16 == 0
    op_a = 0.5 * (a0 + a1) if case.mid else a0
    want = (op_a.T if transa else op_a).dot(b)
    for cw in (n, _small_cw(n)):
        c_d = _c_buffer(m, n, dev)
        before = launch_counts()
        rc = lib.vgpa_ld_gemm(st, int(transa), m, n, k, be._p(a0_d, off), be._p(a1_d, off), lda, be._p(b_d, b_off), ldb, be._p(c_d, BAND), cw)
        assert rc == 0
        torch.cuda.synchronize()
        assert launched(before) == {case.counter: 1}, (launched(before), case.counter)
        assert np.array_equal(_unpack(c_d.cpu().numpy(), m, n, cw), want), (case.name, transa, cw)
    RAN.add((case, transa))


@pytest.mark.parametrize("transa", [False, True], ids=["nn", "tn"])
@pytest.mark.parametrize("case", SEG_CASES, ids=lambda c: c.name)
def test_k_chunk_launches_are_exact(case, transa):
    """vgpa_ld_gemm_chunk on the integer operands: launch j multiplies sub-block j of every rank's block of the operand and continues
    the sums stored in C (`accumulate`); the union of the launches is the whole product, exactly -- and so is ONE segmented launch over
    every k in natural order."""
    import torch
    from legacy_sharded import HipStageBackend
    be = HipStageBackend()
    lib, st, dev = be._lib, be._stream(), torch.device("cuda", 0)
    m, n, k = case.m, case.n, case.world * case.mp
    sub = case.mp // case.chunks
    rng = np.random.default_rng([m, n, k, int(transa)])
    shape = (k, m) if transa else (m, k)
    a, b = exact_operand(rng, shape), exact_operand(rng, (k, n))
    lda, ldb = shape[1] + 2, n + 2
    off, b_off = 2 * lda + 2, 2 * ldb + 2
    a_d, b_d = torch.as_tensor(_view(a, lda, off), device=dev), torch.as_tensor(_view(b, ldb, b_off), device=dev)
    want = (a.T if transa else a).dot(b)
    for cw in (n, _small_cw(n)):
        c_d = _c_buffer(m, n, dev)
        before = launch_counts()
        for j in range(case.chunks):
            a_off = off + (j * sub * lda if transa else j * sub)
            rc = lib.vgpa_ld_gemm_chunk(st, int(transa), m, n, case.world * sub, be._p(a_d, a_off), lda, be._p(b_d, b_off + j * sub * ldb), ldb,
                                        be._p(c_d, BAND), cw, sub // 16, case.mp, int(j > 0))
            assert rc == 0
        torch.cuda.synchronize()
        assert launched(before) == {case.chunk: case.chunks}, (launched(before), case.chunk)
        assert np.array_equal(_unpack(c_d.cpu().numpy(), m, n, cw), want), (case.name, transa, cw)
    c_d = _c_buffer(m, n, dev)
    before = launch_counts()
    assert lib.vgpa_ld_gemm_chunk(st, int(transa), m, n, k, be._p(a_d, off), lda, be._p(b_d, b_off), ldb, be._p(c_d, BAND), n,
                                  case.mp // 16, case.mp, 0) == 0
    torch.cuda.synchronize()
    assert launched(before) == {case.whole: 1}, (launched(before), case.whole)
    assert np.array_equal(_unpack(c_d.cpu().numpy(), m, n, n), want), (case.name, transa)
    RAN.add((case, transa))


# ---- c. the record --------------------------------------------------------------------------------------------------------------

def test_worst_ratios_of_the_module():
    """The worst ratio err_k / max(err_o, 2^-53) per path and quantity over the cases above that ran in this process (after them in file
    order), printed for the log; FACTOR bounds each one.  Where every case of the module ran, every counter of vgpa_ld_launch_counts
    has moved except those launch_gemm cannot reach (rounding section)."""
    for path in dict.fromkeys(p for p, _ in WORST):
        print(f"WORST [{path}]", " ".join(f"{q}={r:.2f}" for (p, q), r in WORST.items() if p == path))
    for level, fused in (("operator level", False), ("fused level", True)):
        worst = {}
        for (p, q), r in WORST.items():
            if p.startswith("fused ") == fused:
                worst[q] = max(worst.get(q, 0.0), r)
        print(f"WORST by quantity, {level}:", " ".join(f"{q}={r:.2f}" for q, r in worst.items()))
    still = sorted(k for k, v in launch_counts().items() if v == 0)
    print("counters that never moved in this process:", still)
    if len(RAN) == len(LD_OPS) + len(LD_FUSED) + 2 * (len(GEMM_CASES) + len(SEG_CASES)):
        assert still == sorted(UNREACHABLE), still
