"""
The marginal backward smoother on the GPU (vgpa_particle_backward_moments).

Three kinds of checks.
  The device against itself, which needs no condition: logw, state, ess and resampled are particle_filter's, bit for bit; two calls give
  the same bits; with ess_fraction = 0 (and with one particle) the moments are particle_moments' and the smoothing ESS its lineage ESS, bit
  for bit; a row of the table at a carried cut is the row above it; a problem's rows do not depend on the batch around it; the cached state
  is untouched.
  The table against the restatement of test_particle_backward_moments_cpu ON THE DEVICE'S OWN HISTORIES -- ancestors and clouds of
  particle_filter(history=True) with the same arguments, whose log_w and state this call reproduces bit for bit, and the replaced
  log-weights of particle_replaced_logw -- one recursion step per cut: row j from the device's own row j + 1, against the longdouble step,
  held to  err_k <= 32 max(err_o, 1)  in units of that module's floor (Bmax from the longdouble step itself).  Nothing chaotic enters: no
  margin condition is needed.
  The moments: at stride 1 and an observation index t_j the replay's states are the filter's cloud, so M1[t_j] = sum_i W^j_i clouds_j[i]
  is one reduction of known numbers: 32 2^-53 (2 + 2 levels(n)) sum W |x| (the product, the tree of the sum; the weights are given).
  Everywhere else against sum W x of the numpy replay with the device's table, |M1 - want| <= 1e-9 sum W |x| and |M2 - want| <= 1e-9 M2:
  the tolerance and scales of test_particle_moments.py, whose replay this call runs untouched (numpy's walk differs from the device's by
  what Lorenz-63 / Lorenz-96 make of an ulp along the path).
Every grid has at most 201 points; the longdouble steps cost n^2 D operations per resampled cut, n <= 300.
"""
import numpy as np
import pytest

import extended_ref as xr
import vgpa_amd as va
from helpers import build_problem
from test_gpu_edge_cases import gpu_context, make_problem
from test_particle_backward_cpu import BCASES, TIGHT, TIGHT_RUNS, tight_case
from test_particle_backward_moments_cpu import (FACTOR, LD, LONG, LONG_N, SIZES, UNIT, errors, long_case, ratio, replay_numpy, smoothing_moments,
                                                step_errors, within)
from test_particle_filter import CACHE_CASES, _batch_context, _ctx, _prior
from test_particle_filter_cpu import FRACTIONS, PLACEMENTS, SEED, SEED_BATCH, batch_case, case, placement_case
from test_problem_batch import _context, _datasets

pytestmark = pytest.mark.gpu

TOL = 1e-9
WALK = ("log_w", "state", "ess", "resampled")
WORST = {"table": 0.0, "final row": 0.0, "ess": 0.0, "m1 at observations": 0.0, "m1": 0.0, "m2": 0.0}      # printed behind the module's last test


@pytest.fixture(scope="module")
def contexts():
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()
    print("worst figures over the module (table, final row, ess, m1 at observations: e_k / max(e_o, 1) or floors; m1, m2: units of their scales):", WORST)


def _same(a, b):
    return all(np.array_equal(a[key], b[key]) for key in a)


def _run(ctx, n, seed, **args):
    """(the call's dict, the filter's dict with its histories, the replaced log-weights); the call is made twice: the same bits"""
    got = ctx.particle_backward_moments(n, seed, **args)
    hlw = ctx.particle_replaced_logw(n)
    assert _same(ctx.particle_backward_moments(n, seed, **args), got)
    args.pop("stride", None)
    flt = ctx.particle_filter(n, seed, history=True, **args)
    for key in WALK:
        assert got[key].dtype == flt[key].dtype and np.array_equal(got[key], flt[key]), key
    return got, flt, hlw


def _history(flt, hlw, obs_t, k=0):
    """problem k's histories as the device holds them, in history_numpy's layout"""
    c = len(obs_t)
    flags = flt["resampled"][k, :c]
    assert np.array_equal(np.isfinite(hlw[k, :c]).all(axis=1), flags.astype(bool)) and np.all(np.isnan(hlw[k, c:]))
    return dict(lw=flt["log_w"][k], obs_t=np.asarray(obs_t, dtype=np.int64), resampled=flags, ancestors=flt["ancestors"][k, :c],
                clouds=flt["clouds"][k, :c], hlw=hlw[k, :c])


def _check(got, hist, q, x, x0, seed, k=0, stride=1, label=""):
    """row k of the call's dict against the restatement on the device's own histories `hist`"""
    c, n, d = hist["obs_t"].size, hist["lw"].size, int(q.dim_d)
    table, ess = got["weights"][k], got["smoothing_ess"][k]
    assert np.all(table[c + 1:] == 0.0) and np.all(ess[c + 1:] == 0.0), label
    table, ess = table[:c + 1], ess[:c + 1]
    assert np.all(np.isfinite(table)) and np.all(table >= 0.0) and np.all(np.abs(table.sum(axis=1) - 1.0) <= 1e-12), label
    # row c: the normalised final weights, one exp, one sum and one division (test_particle_rounding_cpu's floor of a normalised weight)
    lw = np.asarray(hist["lw"], dtype=LD)
    ext = np.exp(lw - lw.max())
    ext = ext / xr._sum(ext, 0)
    w64 = np.exp(hist["lw"] - hist["lw"].max())
    e_k, e_o = errors(table[c], ext, w64 / w64.sum(), (1 + np.abs(lw - lw.max()) + 2 * xr.levels(n)) * ext)
    WORST["final row"] = max(WORST["final row"], ratio(e_k, e_o))
    assert within(e_k, e_o), (label, "row c", e_k, e_o)
    worst = 0.0
    for j in range(c - 1, -1, -1):
        if not hist["resampled"][j]:
            assert np.array_equal(table[j], table[j + 1]) and ess[j] == ess[j + 1], (label, j)
            continue
        e_k, e_o, bmax = step_errors(q, x, seed, hist, j, table[j + 1], table[j], index=k)
        worst = max(worst, ratio(e_k, e_o))
        assert within(e_k, e_o), (label, "row", j, e_k, e_o, float(bmax))
    WORST["table"] = max(WORST["table"], worst)
    # 1 / sum W^2 of the device's own rows: n squares and the tree of their sum, all terms positive
    ext = 1 / xr._sum(np.asarray(table, dtype=LD) ** 2, 1)
    e_k, e_o = errors(ess, ext, 1.0 / np.sum(table * table, axis=1), (3 + 2 * xr.levels(n)) * ext)
    WORST["ess"] = max(WORST["ess"], ratio(e_k, e_o))
    assert within(e_k, e_o), (label, "smoothing_ess", e_k, e_o)
    # the moments
    mom = got["moments"][k]
    states = replay_numpy(q, x, x0, seed, hist, index=k)
    m1, m2, a1 = smoothing_moments(table, states, hist["obs_t"], stride)
    assert mom.shape == (m1.shape[0], 2, d) and np.all(np.isfinite(mom)), label
    e1, e2 = np.abs(mom[:, 0] - m1), np.abs(mom[:, 1] - m2)
    tiny = float(np.finfo(float).tiny)
    WORST["m1"], WORST["m2"] = max(WORST["m1"], float(np.max(e1 / (a1 + tiny)))), max(WORST["m2"], float(np.max(e2 / (m2 + tiny))))
    assert np.all(e1 <= TOL * a1) and np.all(e2 <= TOL * m2), (label, float(np.max(e1 / (a1 + tiny))), float(np.max(e2 / (m2 + tiny))))
    at_obs = 0.0
    if stride == 1:
        for j, t in enumerate(hist["obs_t"]):
            cloud = np.asarray(hist["clouds"][j], dtype=LD).reshape(n, d)
            w = np.asarray(table[j], dtype=LD)[:, None]
            size = (2 + 2 * xr.levels(n)) * xr._sum(w * np.abs(cloud), 0)
            e_k, _ = errors(mom[int(t), 0], xr._sum(w * cloud, 0), mom[int(t), 0], size)
            at_obs = max(at_obs, e_k)
        WORST["m1 at observations"] = max(WORST["m1 at observations"], at_obs)
        assert at_obs <= FACTOR, (label, "M1 at the observations", at_obs)
    print(label, f"stride {stride}: table {worst:.3g}, M1 at observations {at_obs:.3g} floors; smoothing ESS", np.round(ess, 2), "resampled", hist["resampled"])


@pytest.mark.parametrize("ess_fraction", FRACTIONS)
@pytest.mark.parametrize("n_paths", SIZES)
@pytest.mark.parametrize("tag,start", BCASES)
def test_fixture_cases(contexts, tag, start, n_paths, ess_fraction):
    """D = 1, 1, 3, 12, 17, 40, 64 (a drawn start), 12 and 3 (a given one; carried and resampled clouds mixed); n = 1, 17, 65, 257, 300: one
    candidate, a partial block of 16 successors and a partial wave, a wave and one more, a 256-candidate tile and one more, a ragged tile"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    args = dict(ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    got, flt, hlw = _run(ctx, n_paths, SEED, **args)
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    assert got["weights"].shape == (1, obs_t.size + 1, n_paths) and got["smoothing_ess"].shape == (1, obs_t.size + 1)
    _check(got, _history(flt, hlw, obs_t), q, x, s0, SEED, label=f"{tag} n={n_paths} {start} f={ess_fraction}")
    if n_paths == 65:      # stride 3 is [::3] of stride 1, and the table does not leave when it is not asked for
        third = ctx.particle_backward_moments(n_paths, SEED, stride=3, weights=False, **args)
        assert third["weights"] is None and np.array_equal(third["moments"], got["moments"][:, ::3])
        assert np.array_equal(third["smoothing_ess"], got["smoothing_ess"])


@pytest.mark.parametrize("n_paths", sorted({n for n, _ in TIGHT_RUNS}))
@pytest.mark.parametrize("d", TIGHT)
def test_tight_lorenz96_clouds(d, n_paths):
    """Lorenz-96 where the table has something to decide (test_particle_backward_moments_cpu.test_tight_clouds_react_to_the_kernel: a
    mutant of the drift, of 1 / R, of the successor or of the hlw term moves it beyond the bound): D = 12, 40 and 50"""
    q, x = tight_case(d)
    ctx = gpu_context(q)
    args = dict(ess_fraction=1.0, x=x, prior=_prior(q))
    got, flt, hlw = _run(ctx, n_paths, SEED, **args)
    old = ctx.particle_moments(n_paths, SEED, **args)
    ctx.close()
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    assert flt["resampled"][0, 0] == 1
    _check(got, _history(flt, hlw, obs_t), q, x, None, SEED, label=f"tight L96 D={d} n={n_paths}")
    assert got["smoothing_ess"][0, 0] > old["lineage_ess"][0, 0] and got["smoothing_ess"][0, -1] == old["lineage_ess"][0, -1]


@pytest.mark.parametrize("model", LONG)
def test_many_observations(model):
    """20 observations, 128 particles, 16 - 19 resampled cuts in a row: OU, double well, Lorenz-63"""
    q, x = long_case(model)
    ctx = gpu_context(q)
    args = dict(ess_fraction=0.5, x=x, prior=_prior(q))
    got, flt, hlw = _run(ctx, LONG_N, SEED, **args)
    old = ctx.particle_moments(LONG_N, SEED, **args)
    ctx.close()
    obs_t = np.asarray(q.obs_t, dtype=int).ravel()
    assert flt["resampled"][0].sum() >= 10
    _check(got, _history(flt, hlw, obs_t), q, x, None, SEED, label=f"long {model}")
    print(f"long {model}: smoothing ESS", np.round(got["smoothing_ess"][0], 2), "lineage ESS", np.round(old["lineage_ess"][0], 2))
    if model != "L63":
        assert got["smoothing_ess"][0, 0] > old["lineage_ess"][0, 0]
    assert got["smoothing_ess"][0].sum() > old["lineage_ess"][0].sum()


@pytest.mark.parametrize("tag,start", BCASES)
def test_without_resampling_it_is_particle_moments(contexts, tag, start):
    """ess_fraction = 0, and one particle: nothing is resampled, every cut copies, and moments and ESS are particle_moments' bit for bit"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    args = dict(x=x, x0=x0 if start == "given" else None, prior=_prior(q))
    for n, frac, stride in ((17, 0.0, 1), (300, 0.0, 3), (1, 1.0, 1)):
        got, old = ctx.particle_backward_moments(n, SEED, stride=stride, ess_fraction=frac, **args), ctx.particle_moments(n, SEED, stride=stride, ess_fraction=frac, **args)
        assert not got["resampled"].any()
        for key in WALK + ("moments",):
            assert np.array_equal(got[key], old[key]), (tag, n, key)
        assert np.array_equal(got["smoothing_ess"], old["lineage_ess"]), (tag, n)
        assert np.all(got["weights"] == got["weights"][:, -1:]), (tag, n)


@pytest.mark.parametrize("obs_at", PLACEMENTS, ids=lambda t: "t" + "-".join(map(str, t)))
@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_observation_placement(model, d, obs_at):
    """an observation at grid index 0 (x~ is the state of grid index 1), adjacent indices (cuts one step apart), Np - 1 (nothing is
    resampled there: the first cut copies)"""
    q, x = placement_case(model, d, obs_at)
    ctx = gpu_context(q)
    for x0 in (None, np.reshape(np.asarray(q.m0, dtype=float), d) + 0.1):
        for stride in (1, 4):
            got, flt, hlw = _run(ctx, 17, SEED, stride=stride, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q))
            assert flt["resampled"].any()
            _check(got, _history(flt, hlw, obs_at), q, x, x0, SEED, stride=stride, label=f"{model} {obs_at} {'given' if x0 is not None else 'drawn'}")
    ctx.close()


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_with_own_rows(model, d):
    """B = 3 with own theta, isotropic Sigma, observation times, counts, R and H: at a cut of the batch a problem without an observation
    there does nothing, one with a carried cloud copies, one with a resampled cloud recurses; row k is the single-problem restatement of
    index k, rows beyond a problem's count + 1 are 0, and the last problem's result is bit for bit the same beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        runs[first], flt, hlw = _run(ctx, 40, SEED_BATCH, ess_fraction=0.5, x=xs, prior=prior)
        ctx.close()
        assert flt["resampled"].any()
        for k, q in enumerate(probs):
            obs_t = np.asarray(q.obs_t, dtype=int).ravel()
            _check(runs[first], _history(flt, hlw, obs_t, k), q, xs[k], None, SEED_BATCH, k=k, label=f"{model} batch {first} problem {k}")
    for key, val in runs[20].items():
        assert np.array_equal(val[2], runs[50][key][2]), key
    assert not np.array_equal(runs[20]["moments"][0], runs[50]["moments"][0])


@pytest.mark.parametrize("name,method,d,tf,nb", CACHE_CASES, ids=lambda c: str(c))
def test_the_cache_is_not_touched(name, method, d, tf, nb):
    """gradient(None), fetch of mt / st / lamt, energy_parts() and theta_gradient() behind particle_backward_moments(x=None) are bit for bit
    what they are without the call (the orders of test_particle_filter.test_the_cache_is_not_touched)"""
    base, probs, xs = _datasets(name, method, tf, d, nb, False)
    prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))

    def record(ctx):
        return [np.asarray(ctx.gradient(None)), np.asarray(ctx.fetch("mt")), np.asarray(ctx.fetch("st")), np.asarray(ctx.fetch("lamt")),
                np.asarray(ctx.theta_gradient())] + [np.asarray(v) for v in ctx.energy_parts()]

    def run(order):
        ctx = _context(base, probs, nb, 0, obs_t=False)
        ctx.free_energy(xs)
        out = [record(ctx) if step == "record" else ctx.particle_backward_moments(9, 4, prior=prior) for step in order]
        ctx.close()
        return out

    a1, res, a2 = run(["record", "moments", "record"])
    b1, b2 = run(["record", "record"])
    res_c, c1 = run(["moments", "record"])
    assert _same(res, res_c)
    for k in range(len(b1)):
        assert np.array_equal(a1[k], b1[k]) and np.array_equal(c1[k], b1[k]), k
        assert np.array_equal(a2[k], b2[k]), k


def test_errors():
    """the refusals by type -- those of particle_moments and of particle_backward_paths, the new launches' grid limit, the accessor's state
    -- and the context stays usable after each"""
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    usable = lambda: ctx.particle_backward_moments(5, 1, x=xs, prior=(mu, tau))       # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_backward_moments(5, 1)
    with pytest.raises(RuntimeError, match="replaced log-weights"):
        ctx.particle_replaced_logw(5)
    ref = usable()
    assert ctx.particle_replaced_logw(5).shape == (3, ctx.n_obs, 5)
    with pytest.raises(RuntimeError, match="replaced log-weights"):
        ctx.particle_replaced_logw(6)
    ctx.particle_moments(5, 1, x=xs, prior=(mu, tau))
    with pytest.raises(RuntimeError, match="replaced log-weights"):      # (the genealogical call keeps none)
        ctx.particle_replaced_logw(5)
    with pytest.raises(ValueError):
        ctx.particle_backward_moments(0, 1, x=xs)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="stride"):
            ctx.particle_backward_moments(5, 1, stride=bad, x=xs)
    with pytest.raises(ValueError, match="32 bits"):
        ctx.particle_backward_moments(5, 1, stride=2 ** 31, x=xs)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ess_fraction"):
            ctx.particle_backward_moments(5, 1, ess_fraction=bad, x=xs)
    assert _same(usable(), ref)
    # through the C ABI itself, no array of n_paths entries touched: more successors than the new launches' grid.y holds (65535 * 256 / 12 at
    # D = 12) is refused before any work; a null moments, logw or state; smoothing_ess, weights, ess and resampled are optional
    xx, lw, st = np.ascontiguousarray(xs), np.empty((3, 5)), np.empty((3, 5, 12))
    mom = np.full((3, ctx.Np, 2, 12), 3.0)
    call = lambda n, a, b, c: ctx._lib.vgpa_particle_backward_moments(ctx._h, xx.ctypes.data, None, n, 1, 1, 0.5, None, None, a, b, c, None, None, None, None)      # noqa: E731
    assert call(65535 * 256 // 12 + 1, lw.ctypes.data, st.ctypes.data, mom.ctypes.data) == -5
    assert b"backward smoothing is built for at most" in ctx._lib.vgpa_last_error(ctx._h) and np.all(mom == 3.0)
    assert call(5, lw.ctypes.data, st.ctypes.data, None) == -1
    assert call(5, None, st.ctypes.data, mom.ctypes.data) == -1 and call(5, lw.ctypes.data, None, mom.ctypes.data) == -1
    assert call(5, lw.ctypes.data, st.ctypes.data, mom.ctypes.data) == 0
    assert np.array_equal(mom, ctx.particle_backward_moments(5, 1, x=xs)["moments"])
    assert _same(usable(), ref)
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert _same(usable(), ref)
    ctx.close()
    one = gpu_context(make_problem("OU", 1, 21, method="euler")[0])      # D = 1: the row pass's 16 successors per workgroup bind first
    with pytest.raises(NotImplementedError, match="particles per problem"):
        one.particle_backward_moments(65535 * 16 + 1, 1, x=make_problem("OU", 1, 21, method="euler")[1])
    one.close()
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_backward_moments(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_backward_moments(2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_backward_moments(2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


def test_records_of_vargp_and_problem_batch():
    """ProblemBatch.backward_moments and VarGP.backward_moments: one BackwardSmoothingMoments per member, equal to the bare context's rows;
    the 1-D models drop the last axis, and on OU the first stretch keeps a variance where the genealogy's rests on fewer lineages"""
    ps = [build_problem("L96", "euler", 0.5, dim_d=12, seed=100 + k) for k in range(3)]
    for k, p in enumerate(ps):
        p["vgp"].output["s0"] = np.asarray(p["vgp"].output["s0"], dtype=float) * (1.0 + 0.05 * k)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + 0.1 * k
    pb = va.ProblemBatch([p["vgp"] for p in ps])
    x = pb.initialization()
    recs = pb.backward_moments(17, SEED_BATCH, stride=2, x=x)
    prior = (np.stack([v._prior()[0][0] for v in pb.vgps]), np.stack([v._prior()[1][0] for v in pb.vgps]).reshape(3, 12, 12))
    bare = pb._context().particle_backward_moments(17, SEED_BATCH, stride=2, x=pb._stack(x), prior=prior)
    pb.close()
    assert len(recs) == 3
    for k, rec in enumerate(recs):
        c = rec.obs_t.size
        assert isinstance(rec, va.BackwardSmoothingMoments) and len(rec) == 17 and rec.stride == 2
        assert np.array_equal(rec.moments, bare["moments"][k]) and np.array_equal(rec.log_w, bare["log_w"][k])
        assert np.array_equal(rec.weights, bare["weights"][k, :c + 1]) and np.array_equal(rec.smoothing_ess, bare["smoothing_ess"][k, :c + 1])
        assert np.array_equal(rec.var, rec.second - rec.mean ** 2) and rec.smoothing_ess_on_grid().shape == rec.grid.shape and np.isfinite(rec.log_evidence())
    v = build_problem("OU", "euler", 0.5)["vgp"]
    rec = v.backward_moments(33, 3, x=v.initialization())
    old = v.particle_moments(33, 3, x=v.initialization())
    v.invalidate()
    assert rec.mean.shape == rec.var.shape == rec.std.shape == (v.dim_n,) and rec.weights.shape == (rec.obs_t.size + 1, 33)
    assert np.array_equal(rec.log_w, old.log_w) and rec.smoothing_ess[-1] == old.lineage_ess[-1] and np.all(rec.smoothing_ess >= 1.0)
