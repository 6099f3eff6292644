"""
Per-problem observation count, noise and operator (vgpa_set_problem_obs_model / ProblemBatch(own_observations=True)) on the GPU.

Problem k of a batch carries, beside its own dataset (vgpa_set_problem_data), its own observation count M_k (cycling through M,
M - 1, 1: it uses the first M_k entries of its row, the rest is padding of -1 / NaN), its own noise R_k (R (1 + 0.1 (k mod 4)), or a
dense SPD matrix) and its own operator H_k (the identity, a 0/1 mask, or I + 0.1 G_k).  Every problem is checked against the numpy
oracle evaluated on its own truncated dataset with its own R_k, H_k (TOL = 1e-9 relative on F, the gradient, m_t, S_t and E_obs), on
every kernel family the context picks.
"""
import dataclasses

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_MATERIALIZE
from conftest import rel_err
from helpers import SEED, build_problem
from oracle import vgpa_oracle as vo
from test_problem_batch import FAMILIES, _context, _datasets
from test_problem_params import _set_params, _with_params
from test_theta_gradient_cpu import fd_theta_gradient

pytestmark = pytest.mark.gpu

TOL = 1e-9
KINDS = ("count", "noise", "mask", "dense", "all")


def _own_model(p, k, kind):
    """problem k's (M_k, R_k, H_k); R_k / H_k None: the shared one"""
    m = int(np.asarray(p.obs_t).size)
    assert m >= 3
    mk = (m, m - 1, 1)[k % 3] if kind in ("count", "all") else m
    if kind == "count":
        return mk, None, None
    scale = 1.0 + 0.1 * (k % 4)
    if p.single_dim:
        return mk, float(p.obs_noise) * scale, None
    d = p.dim_d
    r = np.reshape(np.asarray(p.obs_noise, dtype=float), (d, d))
    if kind == "noise":
        return mk, r * scale, None
    if kind == "mask":                                # component i is observed unless (i + k) mod 3 = 0
        return mk, r * scale, np.diag(((np.arange(d) + k) % 3 != 0).astype(float))
    s = float(np.mean(np.diag(r)))
    rho = 0.1 * (1 + k % 3)                           # (1 - rho) I + rho 11^T, scaled as _own_sigma scales its dense Sigma
    rk = s * (1.0 + 0.05 * (k % 4)) * ((1.0 - rho) * np.eye(d) + rho * np.ones((d, d)))
    return mk, rk, np.eye(d) + 0.1 * np.random.default_rng(100 + k).standard_normal((d, d))


def _with_obs_model(probs, kind):
    """the oracle problems: problem k on the first M_k of its observations, with its own R_k and H_k"""
    out, counts = [], []
    for k, p in enumerate(probs):
        mk, rk, hk = _own_model(p, k, kind)
        counts.append(mk)
        out.append(dataclasses.replace(p, obs_t=np.asarray(p.obs_t)[:mk], obs_y=np.asarray(p.obs_y)[:mk],
                                       obs_noise=p.obs_noise if rk is None else rk, obs_h=hk))
    if kind in ("count", "all"):
        assert len(set(counts)) >= 2
    return out


def _model_args(full, own, kind):
    """what set_problem_obs_model takes for the batch; inputs the kind leaves shared are passed as None"""
    d, m = full[0].dim_d, int(np.asarray(full[0].obs_t).size)
    n_obs = np.array([np.asarray(q.obs_t).size for q in own], dtype=np.int32) if kind in ("count", "all") else None
    noise = None if kind == "count" else np.stack([np.reshape(q.obs_noise, (d, d)) for q in own])
    h = np.stack([q.obs_h for q in own]) if kind in ("mask", "dense", "all") else None
    assert n_obs is None or n_obs.max() == m
    return dict(n_obs=n_obs, obs_noise=noise, obs_h=h)


def _rows(full, own, own_t, pad):
    """obs_t / obs_y rows of the capacity M; pad: -1 / NaN beyond each problem's count (else the valid entries of the full dataset)"""
    d, m = full[0].dim_d, int(np.asarray(full[0].obs_t).size)
    t = np.stack([np.asarray(q.obs_t, dtype=np.int64) for q in full])
    y = np.stack([np.reshape(q.obs_y, (m, d)) for q in full]).astype(float)
    if pad:
        for k, q in enumerate(own):
            mk = np.asarray(q.obs_t).size
            t[k, mk:] = -1
            y[k, mk:] = np.nan
    return (t if own_t else None), y


def _create(p0, nb, flags=0, obs_noise=None, obs_h=None, m=None):
    d = p0.dim_d
    sig = np.array([[p0.sigma]]) if p0.single_dim else p0.sigma
    m = int(np.asarray(p0.obs_t).size) if m is None else m
    return va.Context(p0.model, p0.method, d, p0.n_pts, p0.dt, sigma=sig, theta=np.atleast_1d(p0.theta), m0=np.atleast_1d(p0.m0),
                      s0=np.reshape(p0.s0, (d, d)), obs_t=np.asarray(p0.obs_t)[:m], obs_y=np.asarray(p0.obs_y)[:m],
                      obs_noise=np.reshape(p0.obs_noise if obs_noise is None else obs_noise, (d, d)), obs_h=obs_h, e0=0.0, batch=nb,
                      flags=flags)


def _set_data(ctx, full, t, y):
    d = full[0].dim_d
    ctx.set_problem_data(obs_t=t, obs_y=y, m0=np.stack([np.atleast_1d(q.m0) for q in full]),
                         s0=np.stack([np.reshape(q.s0, (d, d)) for q in full]),
                         e0=np.array([float(np.asarray(vo.kl0(q))) for q in full]))


def _obs_context(full, own, kind, nb, flags=0, own_t=False, pad=True, model_first=True):
    """full: the datasets of capacity M; own: the same problems on their own count / R / H (the oracle's view)"""
    ctx = _create(full[0], nb, flags)
    t, y = _rows(full, own, own_t, pad)
    if model_first:
        ctx.set_problem_obs_model(**_model_args(full, own, kind))
        _set_data(ctx, full, t, y)
    else:                                  # (no counts in force yet: the rows are validated whole, so they must not be padded)
        assert not pad
        _set_data(ctx, full, t, y)
        ctx.set_problem_obs_model(**_model_args(full, own, kind))
    return ctx


_ORACLE = {}


def _oracle(tag, probs, xs, k):
    """the oracle's sweep of problem k of a batch, once per (batch, problem)"""
    key = (tag, k)
    if key not in _ORACLE:
        _ORACLE[key] = vo.sweep(probs[k], xs[k], faithful=False)
    return _ORACLE[key]


def _check(ctx, probs, xs, checked, tag=None):
    f, g = ctx.sweep(xs)
    f, g = np.atleast_1d(f), np.reshape(g, (len(probs), -1))
    mt, st = np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st"))
    _, _, eobs = ctx.energy_parts()
    eobs = np.atleast_1d(eobs)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    for k in checked:
        f_o, g_o, state = vo.sweep(probs[k], xs[k], faithful=False) if tag is None else _oracle(tag, probs, xs, k)
        print(k, f[k], f_o, eobs[k], state["Eobs"])
        assert abs(f[k] - f_o) <= TOL * abs(f_o), (k, f[k], f_o)
        assert rel_err(g[k], g_o) <= TOL, k
        assert rel_err(mt[k].ravel(), np.ravel(state["mt"])) <= TOL, k
        assert rel_err(st[k].ravel(), np.ravel(state["st"])) <= TOL, k
        assert abs(eobs[k] - state["Eobs"]) <= TOL * abs(state["Eobs"]), (k, eobs[k], state["Eobs"])
    return f, g


def _checked(nb):
    # every problem; of the lane batches every problem of the first and of the last (partial) block of 64
    return range(nb) if nb <= 80 else sorted(set(range(64)) | set(range(64 * ((nb - 1) // 64), nb)))


def _shared_plan(own, nb, flags):
    """the plan of the same context with a shared model of the same family: problem 0's R and H for every problem"""
    ref = _create(own[0], nb, flags, obs_noise=own[0].obs_noise, obs_h=own[0].obs_h, m=None)
    plan = ref.plan()
    ref.close()
    return plan


# L96 D = 48, RK4, 2 problems: above 44 the matrix-core steppers are the symmetric-unit kernels whatever the batch size
CASES = [(name, meth, d, tf, nb, fl, kind) for (name, meth, d, tf, sizes, alt) in FAMILIES for nb in sizes for fl in (0, alt)
         for kind in (KINDS if name not in ("OU", "DW") else KINDS[:2])] + [("L96", "rk4", 48, 0.5, 2, 0, kind) for kind in KINDS]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}{c[2] or ''}-{c[1]}-B{c[4]}-f{c[5]}-{c[6]}")
def test_every_family_against_the_oracle(case):
    name, method, d, tf, nb, flags, kind = case
    base, full, xs = _datasets(name, method, tf, d, nb, False)
    own = _with_obs_model(full, kind)
    ctx = _obs_context(full, own, kind, nb, flags)
    plan = ctx.plan()
    assert plan == _shared_plan(own, nb, flags), plan
    if d == 48 or (d == 40 and nb == 80 and flags == 0):
        assert plan["bwd"] == "mfma" and plan["sym_units"]
    if d == 40 and nb == 80 and flags == 0 and kind in ("count", "noise", "mask"):
        assert plan["packed"] and plan["grad_in_bwd_now"]          # the gradient assembled in the backward kernel, packed jumps
    _check(ctx, own, xs, _checked(nb))
    ctx.close()


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80), ("L63", "rk4", None, 1.0, 520)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_rows_equal_to_the_shared_model_are_bit_identical(case):
    name, method, d, tf, nb = case
    base, full, xs = _datasets(name, method, tf, d, nb, False, nset=1)
    p0 = full[0]
    dd, m = p0.dim_d, int(np.asarray(p0.obs_t).size)
    ref = _create(p0, nb)
    f0, g0 = ref.sweep(xs)
    plan0 = ref.plan()
    ref.close()
    rows = np.tile(np.reshape(p0.obs_noise, (1, dd, dd)), (nb, 1, 1))
    for h in (None, np.tile(np.eye(dd)[None], (nb, 1, 1))):          # (vgpa_config gave no operator: the identity)
        ctx = _create(p0, nb)
        ctx.set_problem_obs_model(n_obs=np.full(nb, m, dtype=np.int32), obs_noise=rows, obs_h=h)
        assert ctx.plan() == plan0
        f1, g1 = ctx.sweep(xs)
        ctx.close()
        assert np.array_equal(f0, f1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80), ("L96", "euler", 12, 0.5, 4), ("L63", "rk4", None, 1.0, 8),
                                  ("L63", "rk4", None, 1.0, 520), ("OU", "heun", None, 2.0, 600)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_padding_is_never_read(case):
    """rows of capacity M with count M - 1 and -1 / NaN in the last entry against rows that were truncated to M - 1 instead"""
    name, method, d, tf, nb = case
    base, full, xs = _datasets(name, method, tf, d, nb, False)
    m = int(np.asarray(full[0].obs_t).size)
    own = [dataclasses.replace(q, obs_t=np.asarray(q.obs_t)[:m - 1], obs_y=np.asarray(q.obs_y)[:m - 1]) for q in _with_obs_model(full, "noise")]
    dd = full[0].dim_d
    noise = np.stack([np.reshape(q.obs_noise, (dd, dd)) for q in own])
    ctx = _create(full[0], nb)
    ctx.set_problem_obs_model(n_obs=np.full(nb, m - 1, dtype=np.int32), obs_noise=noise)
    t, y = _rows(full, own, True, True)
    assert np.all(t[:, m - 1] == -1) and np.all(np.isnan(y[:, m - 1]))
    _set_data(ctx, full, t, y)
    f0, g0 = _check(ctx, own, xs, [0, 1, nb - 1])
    ctx.close()
    ctx = _create(full[0], nb, m=m - 1)
    ctx.set_problem_obs_model(obs_noise=noise)
    _set_data(ctx, full, t[:, :m - 1].copy(), y[:, :m - 1].copy())
    f1, g1 = ctx.sweep(xs)
    ctx.close()
    assert np.array_equal(f0, np.atleast_1d(f1)) and np.array_equal(g0, np.reshape(g1, g0.shape))


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80, "all"), ("L63", "rk4", None, 1.0, 520, "noise")],
                         ids=lambda c: f"{c[0]}-B{c[4]}-{c[5]}")
def test_permuting_the_rows_permutes_the_results(case):
    name, method, d, tf, nb, kind = case
    base, full, xs = _datasets(name, method, tf, d, nb, False)
    own = _with_obs_model(full, kind)
    ctx = _obs_context(full, own, kind, nb)
    f, g = ctx.sweep(xs)
    ctx.close()
    perm = np.random.default_rng(3).permutation(nb)
    ctx = _obs_context([full[i] for i in perm], [own[i] for i in perm], kind, nb)
    fp, gp = ctx.sweep(xs[perm])
    ctx.close()
    assert np.array_equal(fp, f[perm]) and np.array_equal(gp, g[perm])


@pytest.mark.parametrize("case", [("L63", "rk4", None, 1.0, 8), ("L63", "rk4", None, 1.0, 520), ("L96", "euler", 12, 0.5, 4)],
                         ids=lambda c: f"{c[0]}-B{c[4]}")
def test_setter_order(case):
    """data then model, model then data, with per-problem times and per-problem parameters: the oracle, and each other bit for bit"""
    name, method, d, tf, nb = case
    base, full, xs = _datasets(name, method, tf, d, nb, True)
    full = _with_params(full, "diag")
    own = _with_obs_model(full, "all")
    results = []
    for model_first, params_first in ((True, False), (False, False), (False, True)):
        ctx = _create(full[0], nb)
        if params_first:
            _set_params(ctx, full)
        t, y = _rows(full, own, True, False)
        if model_first:
            ctx.set_problem_obs_model(**_model_args(full, own, "all"))
            _set_data(ctx, full, t, y)
        else:
            _set_data(ctx, full, t, y)
            ctx.set_problem_obs_model(**_model_args(full, own, "all"))
        if not params_first:
            _set_params(ctx, full)
        results.append(_check(ctx, own, xs, _checked(nb) if nb <= 80 else [0, 1, 2, nb - 1], tag=("order",) + case))
        ctx.close()
    for f, g in results[1:]:
        assert np.array_equal(f, results[0][0]) and np.array_equal(g, results[0][1])


@pytest.mark.parametrize("case", [("L63", "rk4", None, 1.0, 8, 0), ("L63", "rk4", None, 1.0, 520, 0),
                                  ("L63", "rk4", None, 1.0, 520, FLAG_MATERIALIZE), ("L96", "rk4", 12, 0.5, 4, 0)],
                         ids=lambda c: f"{c[0]}-B{c[4]}-f{c[5]}")
def test_theta_gradient_under_per_problem_observation_models(case):
    name, method, d, tf, nb, flags = case
    base, full, xs = _datasets(name, method, tf, d, nb, False)
    own = _with_obs_model(full, "all")
    ctx = _obs_context(full, own, "all", nb, flags)
    f, g = ctx.sweep(xs)
    got = np.reshape(ctx.theta_gradient(), (nb, -1))
    g2 = ctx.gradient(None)                   # (the cached state survives)
    ctx.close()
    assert np.array_equal(np.reshape(g, (nb, -1)), np.reshape(g2, (nb, -1)))
    for k in (0, 1, 2, nb - 1):
        want = fd_theta_gradient(own[k], xs[k])
        print(k, got[k], want)
        assert rel_err(got[k], want) <= TOL, k


def _member(name, method, tf, d, seed, keep, r_scale):
    """build_problem's wiring on the first `keep` observations (None: all) with the noise scaled by r_scale"""
    p = build_problem(name, method, tf, dim_d=d, seed=seed)
    obs_t = list(p["obs_t"])[:keep] if keep else list(p["obs_t"])
    obs_y = np.asarray(p["obs_y"])[:len(obs_t)]
    noise = r_scale * np.asarray(p["obs_noise"], dtype=float)
    single = p["model"].single_dim
    lik = va.GaussianLikelihood(obs_y, obs_t, float(noise) if single else noise, None, single)
    p["vgp"] = va.VarGP(p["model"], p["m0"], p["s0"], p["fwd"], p["bwd"], lik, p["kl0"], obs_y, obs_t)
    return p


@pytest.mark.parametrize("name,method,tf,d", [("OU", "euler", 2.0, None), ("L96", "rk4", 1.0, 12)])
def test_batch_optimisation_matches_single_problem_runs(name, method, tf, d):
    """three members with different M and R: every member ends where its own VarGP, optimised alone, ends, in as many iterations"""
    ps = [_member(name, method, tf, d, SEED, None, 1.0), _member(name, method, tf, d, SEED + 1, -1, 1.5),
          _member(name, method, tf, d, SEED + 2, 2, 0.7)]
    with pytest.raises(ValueError, match="'R'"):
        va.ProblemBatch([p["vgp"] for p in ps])
    pb = va.ProblemBatch([p["vgp"] for p in ps], own_observations=True)
    opts = {"max_it": 40}
    x, f, stats = pb.optimise(pb.initialization(), opts)
    out = pb.result(1)
    assert out["mt"].shape[0] == pb.dim_n and abs(out["fx"] - f[1]) <= 1e-12 * abs(f[1])
    for k, p in enumerate(ps):
        opt = p["vgp"].device_scg(opts)
        xk, fk = opt(p["vgp"].initialization())
        print(k, f[k], fk, stats["MaxIt"][k], opt.statistics["MaxIt"])
        assert abs(f[k] - fk) <= TOL * abs(fk), (k, f[k], fk)
        assert int(stats["MaxIt"][k]) == int(np.ravel(opt.statistics["MaxIt"])[0])
    pb.close()


def test_errors_keep_the_previous_model():
    base, full, xs = _datasets("L96", "rk4", 0.5, 12, 4, False)
    own = _with_obs_model(full, "all")
    ctx = _obs_context(full, own, "all", 4, own_t=True)      # (its own, padded, obs_t rows)
    m = int(np.asarray(full[0].obs_t).size)
    f0, g0 = ctx.sweep(xs)
    good = _model_args(full, own, "all")
    for bad_count in (0, m + 1):
        n = good["n_obs"].copy()
        n[2] = bad_count
        with pytest.raises(ValueError, match="problem 2"):
            ctx.set_problem_obs_model(n_obs=n, obs_noise=good["obs_noise"], obs_h=good["obs_h"])
    for bad_row in (-np.eye(12), np.ones((12, 12))):              # not positive definite: diagonal, and dense
        r = good["obs_noise"].copy()
        r[2] = bad_row
        with pytest.raises(np.linalg.LinAlgError, match="problem 2"):
            ctx.set_problem_obs_model(n_obs=good["n_obs"], obs_noise=r, obs_h=good["obs_h"])
    with pytest.raises(ValueError):
        ctx.set_problem_obs_model(n_obs=np.ones(3, dtype=np.int32))
    # the stored rows are padded beyond the counts in force: a call that lengthens a prefix onto the padding fails
    with pytest.raises(ValueError, match="problem 1"):
        ctx.set_problem_obs_model(obs_noise=good["obs_noise"], obs_h=good["obs_h"])
    # ... and so does data whose prefix, under the counts in force, is out of order
    t, y = _rows(full, own, True, True)
    t[0, 1] = t[0, 0]
    with pytest.raises(ValueError, match="problem 0"):
        ctx.set_problem_data(obs_t=t, obs_y=y)
    f1, g1 = ctx.sweep(xs)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    ctx.close()
    # 1-D models: no operator, a positive noise
    base, full, xs = _datasets("OU", "euler", 2.0, None, 4, False)
    own = _with_obs_model(full, "noise")
    ctx = _obs_context(full, own, "noise", 4)
    f0, _ = ctx.sweep(xs)
    with pytest.raises(ValueError):
        ctx.set_problem_obs_model(obs_h=np.ones((4, 1, 1)))
    with pytest.raises(ValueError, match="problem 1"):
        ctx.set_problem_obs_model(obs_noise=np.array([[[1.0]], [[0.0]], [[1.0]], [[1.0]]]))
    f1, _ = ctx.sweep(xs)
    assert np.array_equal(f0, f1)
    ctx.close()


def test_ode_only_and_large_d_contexts_refuse():
    ctx = va.Context("NONE", "rk4", 6, 21, 0.01, sigma=np.eye(6), batch=2)
    with pytest.raises(RuntimeError):
        ctx.set_problem_obs_model(n_obs=np.ones(2, dtype=np.int32))
    ctx.close()
    base, full, xs = _datasets("L96", "rk4", 0.5, 72, 2, False, nset=2)
    ctx = _context(base, full, 2, 0, obs_t=False)
    f0, g0 = ctx.sweep(xs)
    with pytest.raises(NotImplementedError):
        ctx.set_problem_obs_model(obs_noise=np.stack([2.0 * np.reshape(q.obs_noise, (72, 72)) for q in full]))
    f1, g1 = ctx.sweep(xs)
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)
    ctx.close()
