"""
GPU suite (-m gpu): every sweep path on dense, adjacent and boundary observations (tests/obs_patterns.py).

The other tests observe every fifth grid point from 2 on: M <= 7, no two observations touch, the last grid point is never observed and
the counter n of quirk Q4 (the covariance diagonal of observation n is read at grid index n, not at t_n) stays among the first few
grid points.  Here every path -- the lane pass, the 16-lane kernels, the role-specialised / symmetric-unit / generic steppers, the
isotropic-Sigma kernels (Q'' stream, gradient waves), D > 64 resident, time-chunked and row-sharded, per-problem observations -- runs
with a jump on every step, on both sides of each of its seams (LDS chunks, time chunks, rank slices), at both ends of the grid and
with n and t_n far apart.

Every case asserts its path first (Context.plan / Context.resident), then F, the gradient per block, lam_t, Psi_t, m_t, S_t and E_obs
against the numpy oracle (lean mode) at TOL = 1e-9, and a second context that runs the same arithmetic on another path at the bound
the existing tests use for that pair.  A lost, doubled or shifted jump moves F far above that tolerance
(test_obs_patterns_cpu.py::test_a_lost_doubled_or_shifted_jump_is_far_above_the_tolerance).
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_KEEP_PSI, FLAG_MATERIALIZE, FLAG_STREAM_LARGE_D, OPT_LD_CHUNK
from conftest import rel_err
from helpers import block_rel_errs
from obs_patterns import lane_seams, pad_rows, patterns, rank_seams, time_chunk_seams, time_slice
from oracle import vgpa_oracle as vo
from test_gpu_edge_cases import fused_grad_switch, gpu_context, make_problem

pytestmark = pytest.mark.gpu
TOL = 1e-9
STATE_KEYS = ("lamt", "psit", "mt", "st")
LANE_T = {"L63": (4, 6), "OU": (16,), "DW": (16,)}        # LDS chunks of the fused pass (T) and of the forward kernel (TT), ode_small.hip

_ORACLE = {}


def _oracle(p, x, key=None):
    """vo.sweep(p, x, faithful=False); with a key, computed once per module run and shared (never modified)"""
    if key is None:
        return vo.sweep(p, x, faithful=False)
    if key not in _ORACLE:
        _ORACLE[key] = vo.sweep(p, x, faithful=False)
    return _ORACLE[key]


def _against_oracle(path, label, p, x, f, g, state=None, eobs=None, key=None):
    """F, the gradient per block, the state arrays and E_obs of ONE problem against the oracle; prints the figures first"""
    f_o, g_o, st = _oracle(p, x, key)
    e_f = abs(f - f_o) / abs(f_o)
    e_ga, e_gb = block_rel_errs(g, g_o, p.n_pts, p.dim_d)
    print("obs-placement %s %s F %.2e gLa %.2e gLb %.2e" % (path, label, e_f, e_ga, e_gb))
    assert e_f <= TOL, (label, "F", f, f_o)
    assert e_ga < TOL and e_gb < TOL, (label, "gradient", e_ga, e_gb)
    for k, got in (state or {}).items():
        assert rel_err(np.reshape(got, np.shape(st[k])), st[k]) < TOL, (label, k)
    if eobs is not None:
        assert abs(eobs - st["Eobs"]) <= TOL * abs(st["Eobs"]), (label, "E_obs", eobs, st["Eobs"])


def _batch_x(x, batch, seed):
    return x[None, :] + 0.02 * np.random.default_rng(seed).standard_normal((batch, x.size))


def _sweep_all(ctx, xb, keys=STATE_KEYS):
    """sweep, E_obs, then the state arrays, all with the leading batch axis"""
    b = ctx.B
    f, g = ctx.sweep(xb if b > 1 else np.reshape(xb, -1))
    eobs = np.atleast_1d(ctx.energy_parts()[2])
    state = {k: np.reshape(ctx.fetch(k), (b, -1)) for k in keys}
    return np.atleast_1d(f), np.reshape(g, (b, -1)), eobs, state


def _problems_against_oracle(path, label, p, xb, out, which, keys=None):
    f, g, eobs, state = out
    for i in which:
        _against_oracle(path, "%s[%d]" % (label, i), p, xb[i], f[i], g[i], {k: v[i] for k, v in state.items()}, eobs[i],
                        key=None if keys is None else keys[i])


# ---------------------------------------------------------------------------------------------------------------- lane pass
@pytest.mark.parametrize("n_pts", ["13", "2T+2"])
@pytest.mark.parametrize("model,method,batch", [("L63", "rk4", 520), ("L63", "heun", 520), ("OU", "rk4", 70), ("OU", "heun", 70),
                                                ("DW", "rk4", 130), ("DW", "heun", 130)])
def test_lane_pass(model, method, batch, n_pts):
    """The fused lane pass (ode_small.hip): the streams travel through LDS in chunks of T grid points (TT in the forward kernel), and
    load_jump's shared-index form (jmT) supplies the jumps.  Np = 13 and 2 T + 2; every pattern, `seams` on both sides of every chunk
    boundary of both kernels.  Every problem against the VGPA_FLAG_MATERIALIZE context (1e-11, as test_fused_lane_pass), problems 0,
    63, 64 and the last against the oracle."""
    d = 3 if model == "L63" else 1
    t_sizes = LANE_T[model]
    n = 13 if n_pts == "13" else 2 * t_sizes[0] + 2
    for name, obs in patterns(n, lane_seams(n, t_sizes)).items():
        label = "%s-%s-%d-%s" % (model, method, n, name)
        p, x = make_problem(model, d, n, method=method, obs_at=obs)
        xb = _batch_x(x, batch, 7 * n + batch)
        ctx, ref = gpu_context(p, batch=batch), gpu_context(p, batch=batch, flags=FLAG_MATERIALIZE)
        assert ctx.plan()["lane_pass"] and ctx.plan()["fwd"] == ctx.plan()["bwd"] == "lane", (label, ctx.plan())
        assert not ref.plan()["lane_pass"], label
        f, g = ctx.sweep(xb)
        assert ctx.resident()["moments"] == "time_major" and ctx.resident()["bwd"] == "none", (label, ctx.resident())
        eobs = np.atleast_1d(ctx.energy_parts()[2])
        out_r = _sweep_all(ref, xb)
        assert np.max(np.abs(f - out_r[0]) / np.abs(out_r[0])) < 1e-11, label
        assert rel_err(g, out_r[1]) < 1e-11, label
        assert rel_err(eobs, out_r[2]) < 1e-12, label
        state = {k: np.reshape(ctx.fetch(k), (batch, -1)) for k in STATE_KEYS}        # (what the pass kept in registers, materialised)
        for k in STATE_KEYS:
            assert rel_err(state[k], out_r[3][k]) < 1e-11, (label, k)
        _problems_against_oracle("lane_pass", label, p, xb, (f, g, eobs, state), sorted({0, 63, 64, batch - 1}))
        ctx.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 16 lanes per problem
@pytest.mark.parametrize("name", ["every", "ends", "run"])
def test_sixteen_lane_kernels(name):
    """D <= 4 below 512 problems: 16 lanes per problem (ode_wave.hip).  The Lorenz-63 sweep of 6 problems against the oracle and the
    workgroup-per-problem kernels (VGPA_FLAG_FORCE_GENERIC: the same expressions, F summed in another order -- 1e-11 as for the lane
    pass's pair); D = 2 and 4 operator-level: obs_energy's dense jumps into solve_bwd (1e-13 against the generic kernels, as
    test_lane_per_problem_steppers)."""
    n, batch = 13, 6
    obs = patterns(n)[name]
    p, x = make_problem("L63", 3, n, method="rk4", obs_at=obs)
    xb = _batch_x(x, batch, 61)
    ctx, ref = gpu_context(p, batch=batch), gpu_context(p, batch=batch, flags=FLAG_FORCE_GENERIC)
    assert ctx.plan()["fwd"] == ctx.plan()["bwd"] == "wave" and not ctx.plan()["lane_pass"], ctx.plan()
    assert ref.plan()["fwd"] == ref.plan()["bwd"] == "generic", ref.plan()
    out, out_r = _sweep_all(ctx, xb), _sweep_all(ref, xb)
    assert np.max(np.abs(out[0] - out_r[0]) / np.abs(out_r[0])) < 1e-11 and rel_err(out[1], out_r[1]) < 1e-11
    _problems_against_oracle("16_lane", "L63-" + name, p, xb, out, range(batch))
    ctx.close(); ref.close()
    for d in (2, 4):
        rng = np.random.default_rng(10 * d + len(name))
        r = np.diag(0.5 + rng.random(d))
        q = vo.Problem(model="NONE", method="rk4", dt=0.01, theta=0.0, sigma=np.eye(d), m0=np.zeros(d), s0=np.eye(d), mu0=np.zeros(d),
                       tau0=np.eye(d), obs_t=obs, obs_y=rng.standard_normal((obs.size, d)), obs_noise=r, n_pts=n, dim_d=d)
        a = 2.0 * np.eye(d) + 0.3 * rng.standard_normal((batch, n, d, d))
        mt = rng.standard_normal((batch, n, d))
        st = 0.2 * np.eye(d) + 0.01 * rng.standard_normal((batch, n, d, d))
        st = st + np.swapaxes(st, 2, 3)
        gm, gs = rng.standard_normal((batch, n, d)), rng.standard_normal((batch, n, d, d))
        res = []
        for flags in (0, FLAG_FORCE_GENERIC):
            c = va.Context("NONE", "rk4", d, n, 0.01, sigma=np.eye(d), obs_t=obs, obs_y=q.obs_y, obs_noise=r, batch=batch, flags=flags)
            assert c.plan()["bwd"] == ("generic" if flags else "wave"), c.plan()
            eobs, jm, js = c.obs_energy(mt, st)
            lam, psi = c.solve_bwd(a, gm, gs, jm, js)
            c.close()
            res.append((eobs, jm, js, lam, psi))
        for got, want in zip(res[0], res[1]):
            assert rel_err(got, want) < 1e-13
        for i in range(batch):
            jm_o, js_o = vo.eobs_gradients(q, mt[i], st[i])
            lam_o, psi_o = vo.solve_bwd("rk4", 0.01, False, a[i], gm[i], gs[i], jm_o, js_o)
            e_o = vo.eobs(q, mt[i], st[i])
            assert abs(res[0][0][i] - e_o) <= TOL * abs(e_o), (d, i)
            assert rel_err(res[0][1][i], jm_o) < TOL and rel_err(res[0][2][i], js_o) < TOL, (d, i)
            assert rel_err(res[0][3][i], lam_o) < TOL and rel_err(res[0][4][i], psi_o) < TOL, (d, i)


# ---------------------------------------------------------------------------------------------------------------- matrix-core and generic steppers
FAMILIES = {"role_specialised": ((12, 24), 0), "symmetric_units": ((40, 52, 33), 0), "generic": ((12,), FLAG_FORCE_GENERIC)}


def _assert_family(family, plan):
    if family == "generic":
        assert plan["fwd"] == plan["bwd"] == "generic", plan
    else:
        assert plan["fwd"] == plan["bwd"] == "mfma" and plan["sym_units"] == (family == "symmetric_units"), plan


@pytest.mark.parametrize("method", ["euler", "heun", "rk2", "rk4"])
@pytest.mark.parametrize("family,d", [(f, d) for f, (ds, _) in FAMILIES.items() for d in ds])
def test_workgroup_steppers(family, d, method):
    """Lorenz-96 on the role-specialised MFMA steppers (D = 12, 24), the symmetric-unit ones (D = 40, 52 and 33, the default there) and
    the generic kernels: Np = 13, patterns `every`, `inner`, `ends`, `tail`, `late` against the oracle."""
    n = 13
    for name in ("every", "inner", "ends", "tail", "late"):
        p, x = make_problem("L96", d, n, method=method, obs_at=patterns(n)[name])
        ctx = gpu_context(p, flags=FAMILIES[family][1])
        _assert_family(family, ctx.plan())
        out = _sweep_all(ctx, x[None, :])
        _problems_against_oracle(family, "%d-%s-%s" % (d, method, name), p, x[None, :], out, [0])
        ctx.close()


@pytest.mark.parametrize("family,d", [("role_specialised", 12), ("symmetric_units", 40), ("generic", 12)])
def test_workgroup_steppers_dense_inputs(family, d):
    """... and one dense Sigma / S0 / R / H case per family with an observation on every grid point: dense matrix jumps on every step."""
    n = 13
    h = np.eye(d) + 0.1 * np.random.default_rng(d).standard_normal((d, d))
    p, x = make_problem("L96", d, n, dense=True, h_op=h, obs_at=patterns(n)["every"])
    ctx = gpu_context(p, flags=FAMILIES[family][1])
    _assert_family(family, ctx.plan())
    out = _sweep_all(ctx, x[None, :])
    _problems_against_oracle(family + "_dense", "%d-every" % d, p, x[None, :], out, [0])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- isotropic Sigma
@pytest.mark.parametrize("n", [2, 3, 5, 13])
@pytest.mark.parametrize("batch", [3, 67])
@pytest.mark.parametrize("d", [40, 35])
def test_isotropic_sigma_kernels(d, batch, n):
    """Sigma = sigma^2 I, RK4, 33 <= D <= 40: packed S_t (the Q4 read of k_obs at every n), Q''_t stored and a separate assembly
    (3 problems), the gradient waves of the backward kernel (67 problems; a two-step pipeline, so every short grid is a case of its
    own) with a jump on every step, at both ends, and with n far from t_n.  Against the VGPA_FLAG_KEEP_PSI context (F identical,
    gradient 1e-12, as test_gradient_waves_of_the_backward_kernel) and the oracle; Psi_t as vgpa_fetch recovers it."""
    done = []
    for name in ("every", "ends", "late"):
        obs = patterns(n)[name]
        if any(np.array_equal(obs, o) for o in done):          # (Np = 2: `ends` is `every`)
            continue
        done.append(obs)
        label = "%d-B%d-%d-%s" % (d, batch, n, name)
        p, x = make_problem("L96", d, n, method="rk4", obs_at=obs, sigma="iso")
        xb = _batch_x(x, batch, 100 * n + batch)
        ctx, ctx_k = gpu_context(p, batch=batch), gpu_context(p, batch=batch, flags=FLAG_KEEP_PSI)
        plan, plan_k = ctx.plan(), ctx_k.plan()
        fused = fused_grad_switch() != "0" if batch >= 64 else fused_grad_switch() == "1"
        assert plan["fwd"] == plan["bwd"] == "mfma" and plan["sym_units"] and plan["bwd_upper"], (label, plan)
        assert plan["store_q"] and plan["packed"] and plan["grad_in_bwd_now"] == fused, (label, plan)
        assert not (plan_k["bwd_upper"] or plan_k["store_q"] or plan_k["packed"] or plan_k["grad_in_bwd_now"]), (label, plan_k)
        f, g = ctx.sweep(xb)
        res = ctx.resident()
        assert res["S"] == "packed" and res["dEs"] == "packed" and res["bwd"] == ("none" if fused else "q"), (label, res)
        eobs = np.atleast_1d(ctx.energy_parts()[2])
        out_k = _sweep_all(ctx_k, xb)
        assert np.array_equal(f, out_k[0]), label
        assert max(rel_err(g[i], out_k[1][i]) for i in range(batch)) < 1e-12, label
        assert rel_err(eobs, out_k[2]) < 1e-13, label
        state = {k: np.reshape(ctx.fetch(k), (batch, -1)) for k in STATE_KEYS}
        assert ctx.resident()["bwd"] == "psi", label                                   # Q''_t -> Psi_t across the fetch
        assert rel_err(state["psit"], out_k[3]["psit"]) < 1e-12 and rel_err(state["lamt"], out_k[3]["lamt"]) < 1e-12, label
        _problems_against_oracle("iso_gradient_waves" if fused else "iso_q_stream", label, p, xb, (f, g, eobs, state),
                                 sorted({0, 31, batch - 1} & set(range(batch))))
        ctx.close(); ctx_k.close()


# ---------------------------------------------------------------------------------------------------------------- D > 64, resident
def _large_x(d, n, method, variant):
    """x of the D > 64 cases: variant 0 is make_problem's, the others perturb it (the same for every pattern: the oracle is shared)"""
    _, x = make_problem("L96", d, n, method=method)
    return x if variant == 0 else x + 0.01 * np.random.default_rng(variant).standard_normal(x.size)


@pytest.mark.parametrize("name", ["every", "inner", "ends", "head", "tail", "run", "late", "seams"])
@pytest.mark.parametrize("d,method,batch", [(72, "rk4", 1), (72, "heun", 1), (72, "rk4", 3), (72, "heun", 3), (130, "rk4", 1), (130, "heun", 1),
                                            (130, "rk4", 3), (130, "heun", 3)])
def test_resident_above_64(d, method, batch, name):
    """64 < D: the per-stage kernels of large_d.hip with the state resident, one problem and a batch of three (problems in grid.z).
    Every problem against the oracle; the last problem of a batch is the x of the single-problem case, whose oracle sweep is shared."""
    n = 13
    obs = patterns(n, rank_seams(n, 3))[name]
    p, _ = make_problem("L96", d, n, method=method, obs_at=obs)
    variants = [0] if batch == 1 else [1, 2, 0]
    xb = np.stack([_large_x(d, n, method, v) for v in variants])
    ctx = gpu_context(p, batch=batch)
    assert ctx.plan()["fwd"] == ctx.plan()["bwd"] == "large_d" and not ctx.streaming, ctx.plan()
    out = _sweep_all(ctx, xb)
    assert ctx.resident()["bwd"] == "psi" and ctx.resident()["S"] == "whole"
    _problems_against_oracle("resident_above_64", "%d-%s-B%d-%s" % (d, method, batch, name), p, xb, out, range(batch),
                             keys=[(d, method, name, v) for v in variants])
    ctx.close()


@pytest.mark.parametrize("model,d,n,batch,flags", [("L96", 72, 260, 1, 0), ("OU", 1, 300, 1, FLAG_MATERIALIZE), ("OU", 1, 300, 70, FLAG_MATERIALIZE),
                                                   ("OU", 1, 300, 1, 0), ("OU", 1, 300, 70, 0)])
def test_more_than_256_observations(model, d, n, batch, flags):
    """M > 256 with an observation on every grid point: the second trip of `for n = tid; n < M; n += 256` in k_obs_fin (D > 64) and in
    the 1-D branch of k_obs.  An OU context takes the fused lane pass by default, whose observation terms come from k_obs_lane;
    VGPA_FLAG_MATERIALIZE keeps the four-kernel path, where F and E_obs are k_obs's (asserted: no lane pass).  The default OU
    contexts run as well: k_obs_lane's loop over 300 observations."""
    p, x = make_problem(model, d, n, obs_at=patterns(n)["every"])
    assert p.obs_t.size == n > 256
    xb = _batch_x(x, batch, n) if batch > 1 else x[None, :]
    ctx = gpu_context(p, batch=batch, flags=flags)
    plan = ctx.plan()
    if d > 64:
        assert plan["fwd"] == plan["bwd"] == "large_d", plan
    else:
        assert plan["fwd"] == plan["bwd"] == "lane" and plan["lane_pass"] == (flags == 0), plan
    out = _sweep_all(ctx, xb)
    if d == 1 and flags:
        assert ctx.resident()["moments"] == "row_major", ctx.resident()          # (the lane pass would have left them time-major)
    path = "m_above_256" + ("" if d > 64 else "_k_obs" if flags else "_lane_pass")
    _problems_against_oracle(path, "%s-%d-B%d" % (model, n, batch), p, xb, out, sorted({0, batch - 1}))
    ctx.close()


def test_per_problem_observations_above_64_are_refused():
    """What the ABI documents as VGPA_ERR_UNSUPPORTED instead of a placement: per-problem observation times or an observation model
    at D > 64, and any per-problem data in the time-chunked sweep.  The shared placement stays in force."""
    n = 13
    pats = patterns(n)
    p, x = make_problem("L96", 72, n, obs_at=pats["every"])
    ctx = gpu_context(p, batch=2)
    xb = _batch_x(x, 2, 5)
    f0, g0 = ctx.sweep(xb)
    t, counts, y_rows = pad_rows([pats["late"], pats["ends"]], n, 72)
    with pytest.raises(NotImplementedError):
        ctx.set_problem_data(obs_t=t, obs_y=y_rows([p.obs_y[pats["late"]], p.obs_y[pats["ends"]]]))
    with pytest.raises(NotImplementedError):
        ctx.set_problem_obs_model(n_obs=counts)
    f1, g1 = ctx.sweep(xb)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    ctx.close()
    st = gpu_context(p, flags=FLAG_STREAM_LARGE_D)
    assert st.streaming
    with pytest.raises(NotImplementedError):
        st.set_problem_data(obs_y=p.obs_y[None])
    with pytest.raises(NotImplementedError):
        st.set_problem_obs_model(n_obs=np.array([2], dtype=np.int32))
    f_s, g_s = st.sweep(x)
    _against_oracle("time_chunked", "after-refusal", p, x, f_s, g_s)
    st.close()


# ---------------------------------------------------------------------------------------------------------------- D > 64, time-chunked
@pytest.mark.parametrize("chunk", [1, 4, 5, 13, 64])
def test_time_chunked_sweep(chunk):
    """VGPA_FLAG_STREAM_LARGE_D at D = 72, Np = 13: observations on a chunk's first and last point (the sweep walks the grid from its
    end in chunks that share their edge point: Np - 1 - k chunk), on every point, and Q4's S[n] from another chunk than m[t_n] (`late`).  Against the resident context (1e-12; the same kernels in the same order per grid point) and
    the oracle.  Psi_t is not kept by this sweep."""
    d, n = 72, 13
    x = _large_x(d, n, "rk4", 0)
    for name, obs in patterns(n, time_chunk_seams(n, chunk)).items():
        if name not in ("every", "late", "seams"):
            continue
        label = "chunk%d-%s" % (chunk, name)
        p, _ = make_problem("L96", d, n, method="rk4", obs_at=obs)
        res, st = gpu_context(p), gpu_context(p, flags=FLAG_STREAM_LARGE_D)
        assert st.streaming and not res.streaming and st.plan()["fwd"] == st.plan()["bwd"] == "large_d", label
        st.set_option(OPT_LD_CHUNK, chunk)
        keys = ("lamt", "mt", "st")
        out, out_r = _sweep_all(st, x[None, :], keys), _sweep_all(res, x[None, :], keys)
        assert abs(out[0][0] - out_r[0][0]) <= 1e-12 * abs(out_r[0][0]), label
        assert rel_err(out[1], out_r[1]) < 1e-12 and rel_err(out[2], out_r[2]) < 1e-12, label
        for k in keys:
            assert rel_err(out[3][k], out_r[3][k]) < 1e-12, (label, k)
        with pytest.raises(NotImplementedError):
            st.fetch("psit")
        # (`seams` differs per chunk size: not shared; `every` and `late` are those of test_resident_above_64)
        _problems_against_oracle("time_chunked", label, p, x[None, :], out, [0], keys=[(d, "rk4", name, 0) if name != "seams" else None])
        res.close(); st.close()


# ---------------------------------------------------------------------------------------------------------------- row-sharded, virtual ranks
@pytest.mark.parametrize("d,n,world", [(96, 13, 3), (128, 11, 2), (128, 10, 4), (96, 13, 1)])
def test_row_sharded_sweep_with_virtual_ranks(d, n, world):
    """vgpa_shard_sweep and vgpa_shard_sweep_sharded on virtual ranks: k_shard_obs gives observation n's m-term to the rank that owns
    t_n and its S-term (Q4) to the rank that owns grid index n.  `every` / `inner`: every rank owns S-terms; `late`: t_n and n on
    different ranks; `seams`: t_lo and t_hi - 1 of every rank; `ends`.  F on every rank and every rank's gradient slice against the
    oracle."""
    from vgpa_amd.large_d import NativeShardedRecursion
    from test_large_d import _virtual_ranks
    names = ("every", "inner", "late", "seams", "ends")
    cases = []
    for name in names:
        p, x = make_problem("L96", d, n, method="rk4", obs_at=patterns(n, rank_seams(n, world))[name])
        f_o, g_o, _ = _oracle(p, x, key=("sharded", d, n, name) if name != "seams" else None)
        cases.append((name, p, x, f_o, g_o[:n * d * d].reshape(n, d, d), g_o[n * d * d:].reshape(n, d), float(np.asarray(vo.kl0(p)))))
    slices = [time_slice(n, r, world) for r in range(world)]
    owner = {t: r for r, (lo, hi) in enumerate(slices) for t in range(lo, hi)}
    if world > 1:          # the branches this test is about are reached: S-terms on every rank, and S[n] on another rank than m[t_n]
        assert {owner[k] for k in range(n)} == set(range(world))              # `every`: observation n's S-term on every rank
        assert max(owner[k] for k in range(n - 2)) >= 1                        # `inner` (M = Np - 2): S-terms beyond rank 0 as well
        assert any(owner[k] != owner[int(t)] for k, t in enumerate(patterns(n)["late"]))

    def body(rank, comm):
        rec = NativeShardedRecursion("rk4", 0.01, d, n, rank=rank, world=world, device=0, comm=comm.table(rank) if world > 1 else None)
        lo, hi = rec.time_slice
        errs = {}
        for name, p, x, f_o, ga_o, gb_o, e0 in cases:
            a_h, b_h = p.split(x)
            args = (p.theta, np.diag(p.sigma), p.m0, p.s0, p.obs_t, p.obs_y, np.diag(p.obs_noise), e0)
            for entry in ("sweep", "sweep_sharded"):
                f, ga, gb = rec.sweep(x, *args) if entry == "sweep" else rec.sweep_sharded(a_h[lo:hi], b_h[lo:hi], *args)
                e = [abs(f - f_o) / abs(f_o), 0.0, 0.0]
                if hi > lo:
                    e[1:] = rel_err(ga.cpu().numpy(), ga_o[lo:hi]), rel_err(gb.cpu().numpy(), gb_o[lo:hi])
                errs[(name, entry)] = e
        rec.close()
        return (lo, hi), errs

    out, fails, _ = _virtual_ranks(world, body)
    assert not any(fails), fails
    assert [o[0] for o in out] == slices                 # (the seams were computed from the slices the library hands out)
    for rank, (_, errs) in enumerate(out):
        for (name, entry), e in errs.items():
            print("obs-placement row_sharded %d-%d-w%d-%s-%s[rank %d] F %.2e gLa %.2e gLb %.2e" % (d, n, world, name, entry, rank, *e))
    for rank, (_, errs) in enumerate(out):
        for key, e in errs.items():
            assert max(e) < TOL, (rank, key, e)


# ---------------------------------------------------------------------------------------------------------------- per-problem observations
PER_PROBLEM = {  # model, D, batch, Sigma form, flags of the context, flags of the other path, bound of the pair on (F, gradient)
    "lane_pass": ("L63", 3, 520, "diag", 0, FLAG_MATERIALIZE, (1e-11, 1e-11)),
    "16_lane": ("L63", 3, 6, "diag", 0, FLAG_FORCE_GENERIC, (1e-11, 1e-11)),
    "mfma_12": ("L96", 12, 5, "diag", 0, FLAG_FORCE_GENERIC, (1e-11, 1e-11)),
    "iso_40": ("L96", 40, 67, "iso", 0, FLAG_KEEP_PSI, (0.0, 1e-12)),
}


@pytest.mark.parametrize("path", list(PER_PROBLEM))
def test_per_problem_observations(path):
    """vgpa_set_problem_obs_model(n_obs) + vgpa_set_problem_data(obs_t, obs_y): problem k observes at pattern k mod 7 (`every` ...
    `late`), rows of capacity Np padded with -1 / NaN.  load_jump's per-problem index map on the lane pass and the 16-lane kernels,
    the per-problem jump tables of the MFMA steppers and of the packed isotropic path.  The first problem of every pattern against the
    oracle on its own observations, all problems against the same batch on another path.  The bounds of the pairs: MATERIALIZE and
    KEEP_PSI as the existing tests state them; FORCE_GENERIC evaluates the same recursion with other summation orders -- 13 steps of
    <= 4 stages of length-D sums are ~1e3 roundings of 1.1e-16 each, 1e-13, and 1e-11 leaves two decades for cancellation in F."""
    model, d, batch, sigma, flags, other, (tol_f, tol_g) = PER_PROBLEM[path]
    n = 13
    pats = list(patterns(n).values())
    assert len(pats) == 7
    base, x = make_problem(model, d, n, method="rk4", obs_at=patterns(n)["every"], sigma=sigma)
    xb = _batch_x(x, batch, 300 + batch)
    rng = np.random.default_rng(batch)
    rows = [pats[k % 7] for k in range(batch)]
    ys = [base.obs_y[rows[k]] + 0.1 * rng.standard_normal((rows[k].size, d)) for k in range(batch)]
    own = [dataclasses.replace(base, obs_t=rows[k], obs_y=ys[k]) for k in range(batch)]
    t, counts, y_rows = pad_rows(rows, n, d)
    y = y_rows(ys)
    assert np.all(t[1, n - 2:] == -1) and np.all(np.isnan(y[2, 2:]))
    outs = []
    for fl in (flags, other):
        ctx = gpu_context(base, batch=batch, flags=fl)
        plan = ctx.plan()
        ctx.set_problem_obs_model(n_obs=counts)
        ctx.set_problem_data(obs_t=t, obs_y=y)
        assert ctx.plan() == plan, (path, fl)
        if fl == flags:
            if path == "lane_pass":
                assert plan["lane_pass"] and plan["bwd"] == "lane", plan
            elif path == "16_lane":
                assert plan["fwd"] == plan["bwd"] == "wave", plan
            elif path == "mfma_12":
                assert plan["fwd"] == plan["bwd"] == "mfma" and not plan["sym_units"], plan
            else:
                assert plan["bwd"] == "mfma" and plan["sym_units"] and plan["packed"], plan
                assert plan["grad_in_bwd_now"] == (fused_grad_switch() != "0"), plan
        else:
            assert (plan["bwd"] == "generic") if other == FLAG_FORCE_GENERIC else not (plan["lane_pass"] or plan["packed"]), plan
        outs.append(_sweep_all(ctx, xb))
        ctx.close()
    got, alt = outs
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert np.max(np.abs(got[0] - alt[0]) / np.abs(alt[0])) <= tol_f, path
    assert max(rel_err(got[1][i], alt[1][i]) for i in range(batch)) < tol_g, path
    for k in range(7 if batch >= 7 else batch):
        _against_oracle("per_problem_" + path, "pattern%d" % k, own[k], xb[k], got[0][k], got[1][k], {key: v[k] for key, v in got[3].items()},
                        got[2][k])
