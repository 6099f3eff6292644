"""
Batches of independent datasets (vgpa_set_problem_data / ProblemBatch) on the GPU.

Every problem k of a batch carries its own dataset -- observation values (and, where asked, times), m0, S0, e0 -- built with
build_problem's wiring from its own seed, and its own x.  Problems are checked against the numpy oracle evaluated on problem k's
data (TOL = 1e-9 relative, as the rest of the suite), on every kernel family the context picks at that size.
"""
import json
import os

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd._lib import FLAG_FORCE_GENERIC, FLAG_MATERIALIZE
from conftest import GOLDEN_DIR, rel_err
from helpers import SEED, build_problem
from oracle import vgpa_oracle as vo

pytestmark = pytest.mark.gpu

TOL = 1e-9
N_DATASETS = 4          # distinct datasets (seeds) per batch; problem k takes dataset k % N_DATASETS and a problem-own m0 shift


def _oracle_problem(p, name, method, obs_t=None, obs_y=None, m0=None, s0=None):
    single = name in ("OU", "DW")
    model = p["model"]
    d = 1 if single else model.sample_path.shape[-1]
    theta = np.asarray(model.theta, dtype=float)
    return vo.Problem(model=name, method=method.lower(), dt=float(p["fwd"].dt),
                      theta=float(theta) if theta.ndim == 0 else theta,
                      sigma=float(model.sigma) if single else np.asarray(model.sigma, dtype=float),
                      m0=p["m0"] if m0 is None else m0, s0=p["s0"] if s0 is None else s0, mu0=p["mu0"], tau0=p["tau0"],
                      obs_t=np.asarray(p["obs_t"] if obs_t is None else obs_t, dtype=np.int64),
                      obs_y=np.asarray(p["obs_y"] if obs_y is None else obs_y), obs_noise=p["obs_noise"],
                      n_pts=p["vgp"].dim_n, dim_d=d)


def _datasets(name, method, tf, d, nb, vary_t, nset=N_DATASETS):
    """nb oracle problems (own data each) and their x; dataset j from seed SEED + j, observation times shifted by j % 3 grid
    points when vary_t (same count M), m0 shifted by 0.01 k and S0 scaled by 1 + 0.05 (k mod 7) for problem k (build_problem's S0
    is 0.2 I whatever the seed: the scale makes every problem's initial covariance its own)."""
    base = [build_problem(name, method, tf, dim_d=d, seed=SEED + j) for j in range(min(nset, nb))]
    probs, xs = [], []
    rng = np.random.default_rng(7)
    for k in range(nb):
        p = base[k % len(base)]
        j = k % len(base)
        n = p["vgp"].dim_n
        obs_t = np.asarray(p["obs_t"], dtype=np.int64)
        if vary_t:
            obs_t = np.minimum(obs_t + (j % 3), n - 1)
            obs_t = np.unique(obs_t)
            assert obs_t.size == len(p["obs_t"])
        m0 = np.asarray(p["m0"], dtype=float) + 0.01 * k
        s0 = np.asarray(p["s0"], dtype=float) * (1.0 + 0.05 * (k % 7))
        probs.append(_oracle_problem(p, name, method, obs_t=obs_t, m0=float(m0) if np.ndim(m0) == 0 else m0,
                                     s0=float(s0) if np.ndim(s0) == 0 else s0))
        x0 = p["vgp"].initialization()
        xs.append(x0 + 1e-3 * rng.standard_normal(x0.size))
    return base[0], probs, np.stack(xs)


def _context(base, probs, nb, flags=0, obs_t=True):
    p0 = probs[0]
    d = p0.dim_d
    single = p0.single_dim
    sig = np.array([[p0.sigma]]) if single else p0.sigma
    ctx = va.Context(p0.model, p0.method, d, p0.n_pts, p0.dt, sigma=sig, theta=np.atleast_1d(p0.theta), m0=np.atleast_1d(p0.m0),
                     s0=np.reshape(p0.s0, (d, d)), obs_t=p0.obs_t, obs_y=p0.obs_y, obs_noise=np.reshape(p0.obs_noise, (d, d)),
                     e0=0.0, batch=nb, flags=flags)
    m = p0.obs_t.size
    ctx.set_problem_data(obs_t=np.stack([q.obs_t for q in probs]) if obs_t else None,
                         obs_y=np.stack([np.reshape(q.obs_y, (m, d)) for q in probs]),
                         m0=np.stack([np.atleast_1d(q.m0) for q in probs]),
                         s0=np.stack([np.reshape(q.s0, (d, d)) for q in probs]),
                         e0=np.array([float(np.asarray(vo.kl0(q))) for q in probs]))
    return ctx


def _check_against_oracle(ctx, probs, xs, checked):
    f, g = ctx.sweep(xs)
    f, g = np.atleast_1d(f), np.reshape(g, (len(probs), -1))
    mt, st = np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st"))
    e0, _, _ = ctx.energy_parts()
    for k in checked:
        f_o, g_o, state = vo.sweep(probs[k], xs[k], faithful=False)
        assert abs(f[k] - f_o) <= TOL * abs(f_o), (k, f[k], f_o)
        assert rel_err(g[k], g_o) <= TOL, k
        assert rel_err(mt[k].ravel(), np.ravel(state["mt"])) <= TOL, k
        assert rel_err(st[k].ravel(), np.ravel(state["st"])) <= TOL, k
        assert abs(np.atleast_1d(e0)[k] - state["E0"]) <= 1e-12 * max(1.0, abs(state["E0"])), k
    return f, g


# (model, method, D, tf, batch sizes, the flag of the second kernel family)
FAMILIES = [
    ("OU", "heun", None, 2.0, (8, 600), FLAG_MATERIALIZE),
    ("DW", "rk2", None, 2.0, (8, 600), FLAG_MATERIALIZE),
    ("L63", "rk4", None, 1.0, (8, 520), FLAG_MATERIALIZE),
    ("L96", "euler", 12, 0.5, (4, 80), FLAG_FORCE_GENERIC),
    ("L96", "rk4", 17, 0.5, (4, 80), FLAG_FORCE_GENERIC),
    ("L96", "rk4", 40, 0.5, (4, 80), FLAG_FORCE_GENERIC),
]
CASES = [(name, meth, d, tf, nb, fl) for (name, meth, d, tf, sizes, alt) in FAMILIES for nb in sizes for fl in (0, alt)]


def _ids(c):
    return f"{c[0]}{c[2] or ''}-{c[1]}-B{c[4]}-f{c[5]}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("vary_t", [False, True], ids=["shared_t", "own_t"])
def test_every_family_against_the_oracle(case, vary_t):
    name, method, d, tf, nb, flags = case
    base, probs, xs = _datasets(name, method, tf, d, nb, vary_t)
    ctx = _context(base, probs, nb, flags, obs_t=vary_t)
    # every problem; of the lane batches (several hundred problems) every problem of the first and of the last (partial) block of 64
    checked = range(nb) if nb <= 80 else sorted(set(range(64)) | set(range(64 * ((nb - 1) // 64), nb)))
    _check_against_oracle(ctx, probs, xs, checked)
    ctx.close()


def test_above_d64_per_problem_values_and_moments():
    base, probs, xs = _datasets("L96", "rk4", 0.5, 72, 3, False, nset=3)
    assert len({np.asarray(q.s0).tobytes() for q in probs}) == 3 and len({np.asarray(q.m0).tobytes() for q in probs}) == 3
    ctx = _context(base, probs, 3, 0, obs_t=False)
    _check_against_oracle(ctx, probs, xs, [0, 1, 2])
    with pytest.raises(NotImplementedError):
        ctx.set_problem_data(obs_t=np.stack([q.obs_t for q in probs]))
    ctx.close()


@pytest.mark.parametrize("case", [("L96", "rk4", 17, 0.5, 8), ("L63", "rk4", None, 1.0, 8), ("L63", "rk4", None, 1.0, 520),
                                  ("OU", "euler", None, 2.0, 600)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_permuting_the_problems_permutes_the_results(case):
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, True)
    ctx = _context(base, probs, nb, 0, obs_t=True)
    f, g = ctx.sweep(xs)
    perm = np.random.default_rng(3).permutation(nb)
    ctx.close()
    ctx = _context(base, [probs[i] for i in perm], nb, 0, obs_t=True)
    fp, gp = ctx.sweep(xs[perm])
    assert np.array_equal(fp, f[perm]) and np.array_equal(gp, g[perm])
    ctx.close()


@pytest.mark.parametrize("case", [("L96", "rk4", 40, 0.5, 80), ("L96", "rk4", 17, 0.5, 4), ("L63", "rk4", None, 1.0, 520),
                                  ("L63", "rk4", None, 1.0, 8), ("OU", "heun", None, 2.0, 600)], ids=lambda c: f"{c[0]}-B{c[4]}")
def test_rows_equal_to_the_shared_data_are_bit_identical(case):
    name, method, d, tf, nb = case
    base, probs, xs = _datasets(name, method, tf, d, nb, False, nset=1)
    p0 = probs[0]                                       # every row below = the shared configuration
    dd = p0.dim_d
    sig = np.array([[p0.sigma]]) if p0.single_dim else p0.sigma
    e0 = float(np.asarray(vo.kl0(p0)))
    kw = dict(sigma=sig, theta=np.atleast_1d(p0.theta), m0=np.atleast_1d(p0.m0), s0=np.reshape(p0.s0, (dd, dd)), obs_t=p0.obs_t,
              obs_y=p0.obs_y, obs_noise=np.reshape(p0.obs_noise, (dd, dd)), e0=e0, batch=nb)
    ref = va.Context(p0.model, p0.method, dd, p0.n_pts, p0.dt, **kw)
    f0, g0 = ref.sweep(xs)
    ref.close()
    m = p0.obs_t.size
    ctx = va.Context(p0.model, p0.method, dd, p0.n_pts, p0.dt, **kw)
    ctx.set_problem_data(obs_t=np.tile(p0.obs_t, (nb, 1)), obs_y=np.tile(np.reshape(p0.obs_y, (1, m, dd)), (nb, 1, 1)),
                         m0=np.tile(np.atleast_1d(p0.m0), (nb, 1)), s0=np.tile(np.reshape(p0.s0, (1, dd, dd)), (nb, 1, 1)),
                         e0=np.full(nb, e0))
    f1, g1 = ctx.sweep(xs)
    ctx.close()
    assert np.array_equal(f0, f1) and np.array_equal(g0, g1)


def test_full_size_batch_has_no_cross_talk():
    """64 problems of L96 D = 40, RK4, Np = 1001 on the bench kernels: problem 0 carries the dataset (and x) behind the anchors'
    l96d40_rk4_full_p, the other 63 datasets of other seeds."""
    a = json.load(open(os.path.join(GOLDEN_DIR, "anchors.json")))["l96d40_rk4_full_p"]
    nb = 64
    p0 = build_problem("L96", "RK4", a["tf"], a["dt"], 40)
    others = [build_problem("L96", "RK4", a["tf"], a["dt"], 40, seed=SEED + 1 + j) for j in range(3)]
    x0 = p0["vgp"].initialization()
    xs = [x0 + 0.05 * np.random.default_rng(0).standard_normal(x0.size)]
    vgps = [p0["vgp"]]
    for k in range(1, nb):
        q = others[k % 3]
        xq = q["vgp"].initialization()
        xs.append(xq + 0.05 * np.random.default_rng(100 + k).standard_normal(xq.size))
        vgps.append(q["vgp"])
    pb = va.ProblemBatch(vgps)
    f, g = pb.sweep(np.stack(xs))
    assert abs(f[0] - a["F"]) <= TOL * abs(a["F"])
    assert abs(np.linalg.norm(g[0]) - a["grad_norm"]) <= TOL * a["grad_norm"]
    assert abs(np.abs(g[0]).max() - a["grad_absmax"]) <= TOL * a["grad_absmax"]
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(g))
    pb.close()


@pytest.mark.parametrize("name,method,tf,d", [("OU", "euler", 2.0, None), ("L96", "rk4", 1.0, 12)])
def test_problem_batch_optimisation_matches_single_problem_runs(name, method, tf, d):
    ps = [build_problem(name, method, tf, dim_d=d, seed=SEED + j) for j in range(4)]
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    opts = {"max_it": 40}
    x, f, stats = pb.optimise(pb.initialization(), opts)
    assert x.shape == (4, pb.len_x) and f.shape == (4,)
    for k, p in enumerate(ps):
        xk, fk = p["vgp"].device_scg(opts)(p["vgp"].initialization())
        assert abs(f[k] - fk) <= 1e-8 * abs(fk), (k, f[k], fk)
    out = pb.result(2)
    assert set(out) >= {"fx", "at", "bt", "m0", "s0", "mt", "st", "lamt", "psit", "Efx", "Edf"}
    assert out["fx"] == f[2]
    pb.close()


def _batch_with_golden_problem_0(name, method, d, nb, n_other=3):
    """problem 0: the dataset of the recorded reference optimisation (build_problem at SEED, tf = 10); problems 1.. cycle over
    n_other datasets of other seeds"""
    p0 = build_problem(name, method, 10.0, 0.01, d)
    others = [build_problem(name, method, 10.0, 0.01, d, seed=SEED + 1 + j) for j in range(n_other)]
    members = [p0] + [others[(k - 1) % n_other] for k in range(1, nb)]
    return p0, others, members


def test_problem_batch_reproduces_the_recorded_small_config_optimisation():
    """BASELINE configs[0] (OU, Euler, lane kernels): problem 0 of a batch of 4 follows the reference's complete SCG run
    (tests/golden/scg_full_config1.json) under the checks test_device_scg.py applies to it; every other problem, on data of its own,
    ends where a single-problem DeviceSCG run on its dataset ends."""
    ref = json.load(open(os.path.join(GOLDEN_DIR, "scg_full_config1.json")))
    n_it = ref["MaxIt_stat"]
    p0, others, members = _batch_with_golden_problem_0("OU", "Euler", None, 4)
    pb = va.ProblemBatch([p["vgp"] for p in members])
    opts = {"max_it": ref["max_it"], "x_tol": 1e-6, "f_tol": 1e-8, "display": False}
    x, f, st = pb.optimise(pb.initialization(), dict(opts))
    assert int(st["MaxIt"][0]) == n_it
    assert np.allclose(np.asarray(st["fx"])[:n_it, 0], ref["fx_trace"], rtol=1e-7, atol=0)
    assert abs(f[0] - ref["f_final"]) <= 1e-8 * abs(ref["f_final"])
    assert abs(np.linalg.norm(x[0]) - ref["x_norm"]) <= 1e-7 * ref["x_norm"]
    for k in range(1, 4):
        v = members[k]["vgp"]
        _, fk = v.device_scg(dict(opts))(v.initialization())
        assert abs(f[k] - fk) <= 1e-8 * abs(fk), (k, f[k], fk)
    assert len({round(float(v), 6) for v in f}) == 4
    pb.close()


def test_problem_batch_reproduces_the_recorded_baseline_optimisation():
    """BASELINE configs[2] (L96, D = 40, RK4, Np = 1001): problem 0 of a batch of 64 -- the fragment-cover steppers with the fused
    backward + gradient kernel -- follows the reference's complete SCG run (tests/golden/scg_full_config3.json) under the checks
    test_device_scg.py applies to the device optimiser; problems 1..63 run on three other datasets, each ending where a
    single-problem DeviceSCG run on its dataset ends."""
    ref = json.load(open(os.path.join(GOLDEN_DIR, "scg_full_config3.json")))
    n_it = ref["MaxIt_stat"]
    nb = 64
    p0, others, members = _batch_with_golden_problem_0("L96", "RK4", 40, nb)
    pb = va.ProblemBatch([p["vgp"] for p in members])
    opts = {"max_it": 500, "x_tol": 1e-6, "f_tol": 1e-8, "display": False}
    x, f, st = pb.optimise(pb.initialization(), dict(opts))
    ref_fx = np.asarray(ref["fx_trace"], dtype=float)[:n_it]
    moving = np.nonzero(np.abs(ref_fx - ref["f_final"]) > 1e-9 * abs(ref["f_final"]))[0]
    stall = int(moving[-1]) + 1 if moving.size else 0
    n_dev = int(st["MaxIt"][0])
    assert stall + 10 <= n_dev <= stall + 30, (stall, n_dev)       # past the shared iterations only rejected steps
    b = np.asarray(st["beta"], dtype=float)[:n_dev, 0]
    assert np.array_equal(b[stall + 1:], 4.0 * b[stall:-1])
    n_cmp = min(n_dev, n_it)
    assert n_cmp >= stall + 10
    fx0 = np.asarray(st["fx"], dtype=float)[:, 0]
    assert np.all(np.abs(fx0[n_cmp:n_dev] - ref["f_final"]) <= 1e-9 * abs(ref["f_final"]))
    assert np.allclose(fx0[:n_cmp], ref["fx_trace"][:n_cmp], rtol=1e-9, atol=0)
    assert abs(f[0] - ref["f_final"]) <= 1e-9 * abs(ref["f_final"])
    for j, q in enumerate(others):
        v = q["vgp"]
        _, fq = v.device_scg(dict(opts))(v.initialization())
        for k in range(1 + j, nb, len(others)):
            assert abs(f[k] - fq) <= 1e-8 * abs(fq), (k, f[k], fq)
    pb.close()


def test_errors_map_to_the_wrappers_exceptions():
    base, probs, xs = _datasets("L96", "rk4", 0.5, 12, 4, False)
    ctx = _context(base, probs, 4, 0, obs_t=False)
    m = probs[0].obs_t.size
    with pytest.raises(ValueError):
        ctx.set_problem_data(m0=np.zeros((3, 12)))
    with pytest.raises(ValueError):
        ctx.set_problem_data(obs_y=np.zeros((4, m, 11)))
    bad = np.stack([q.obs_t for q in probs])
    bad[2, [0, 1]] = bad[2, [1, 0]]
    with pytest.raises(ValueError):
        ctx.set_problem_data(obs_t=bad)
    bad = np.stack([q.obs_t for q in probs])
    bad[1, -1] = probs[0].n_pts
    with pytest.raises(ValueError):
        ctx.set_problem_data(obs_t=bad)
    s0 = np.stack([np.reshape(q.s0, (12, 12)) for q in probs])
    s0[3] = -np.eye(12)
    ctx.set_problem_data(s0=s0)
    with pytest.raises(np.linalg.LinAlgError):
        ctx.sweep(xs)
    ctx.close()
