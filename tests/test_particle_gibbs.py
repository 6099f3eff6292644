"""
The conditional particle filter with ancestor sampling and the particle Gibbs chain on the GPU (vgpa_particle_conditional,
VarGP.particle_gibbs).

Two kinds of checks, as in test_particle_backward.py.
  The device against itself, which needs no condition: the four bit identities of vgpa_hip.h -- the trajectory is the reference wherever its
  slot is 0, passes through the run's own cloud at every observation and ends in the run's final particle; with one particle it is the
  reference --, clouds[j][0] is the reference's point, without resampling the slots >= 1 are particle_filter's bit for bit, two calls
  give the same bits, a batch equals its single runs, and the neighbouring entry points return what they return without it.
  Against the restatement of test_particle_gibbs_cpu, whose margin conditions hold for every run here
  (test_particle_gibbs_cpu.test_margin_conditions: ancestor draws >= 1e-8, multinomial thresholds >= 1e-9 S, the pick >= 1e-7 S): the
  slot table and the ancestors exactly; logw and the trajectory with |got - want| <= 1e-9 (scale + tiny), scale = the largest |value|,
  the yardstick of test_particle_backward.py.
Every grid has at most 101 points; the references are trajectories of the particle_paths restatement at another seed.
"""
import numpy as np
import pytest

import vgpa_amd as va
from conftest import load_golden
from helpers import problem_from_golden
from test_gpu_edge_cases import gpu_context, make_problem
from test_particle_filter import _batch_context, _ctx, _prior, contexts      # noqa: F401
from test_particle_filter_cpu import MARGIN, SEED, SEED_BATCH, batch_case, case
from test_particle_gibbs_cpu import (BOUNDARY, GAP, TIGHT, TIGHT_PARTICLES, batch_reference, check_identities, gibbs_runs, reference,
                                     reference_path, tight_case, tight_reference, tight_reference_path)
from vgpa_amd.particles import theta_conditional, theta_draw

pytestmark = pytest.mark.gpu

TOL = 1e-9
TINY = float(np.finfo(float).tiny)


def _close(got, want, label):
    scale = np.max(np.abs(want)) + TINY
    err = float(np.max(np.abs(got - want)) / scale)
    print(label, "worst |got - want| / scale:", err)
    assert np.all(np.abs(got - want) <= TOL * scale), (label, err)


def _against_restatement(got, hist, path, table, k=0, label=""):
    """row k of Context.particle_conditional(history=True)'s dict against one restatement"""
    c, n = hist["ess"].size, hist["lw"].size
    assert np.array_equal(got["resampled"][k, :c], hist["resampled"]), (label, got["resampled"][k], hist["resampled"])
    assert np.array_equal(got["ancestors"][k, :c], hist["ancestors"]), (label, np.argwhere(got["ancestors"][k, :c] != hist["ancestors"])[:4])
    assert np.array_equal(got["slots"][k, :c + 1], table) and np.all(got["slots"][k, c + 1:] == -1), (label, got["slots"][k], table)
    assert got["log_w"].shape[1] == n
    _close(got["log_w"][k], hist["lw"], label + " logw")
    _close(got["trajectory"][k], path, label + " trajectory")
    _close(got["state"][k], hist["state"], label + " state")


def _identities(got, q, ref, k=0):
    """the bit identities on the device's own results"""
    c = int(np.asarray(q.obs_t).size)
    hist = dict(obs_t=np.asarray(q.obs_t, dtype=np.int64).ravel(), clouds=got["clouds"][k, :c], state=got["state"][k])
    check_identities(q, hist, got["trajectory"][k], got["slots"][k, :c + 1].astype(np.int64), ref)


def _same(a, b):
    return all((a[key] is None and b[key] is None) or np.array_equal(a[key], b[key], equal_nan=a[key].dtype.kind == "f") for key in a)


@pytest.mark.parametrize("tag,start,n_paths,ess_fraction", gibbs_runs())
def test_conditional_filter(contexts, tag, start, n_paths, ess_fraction):       # noqa: F811
    """D = 1, 3 (one lane per slot), 12, 17, 40, 64 (the matrix-core walk: NT = 16, 32, 48, 64); one particle, a partial wave, a second
    workgroup above D = 4, a second pass of the prefix sums; never, sometimes and always resampled"""
    q, x, x0 = case(tag)
    ctx = _ctx(contexts, tag)
    s0 = x0 if start == "given" else None
    ref = reference_path(tag, start)
    label = f"{tag} n={n_paths} {start} f={ess_fraction}"
    args = dict(ess_fraction=ess_fraction, x=x, x0=s0, prior=_prior(q))
    got = ctx.particle_conditional(ref, n_paths, SEED, history=True, **args)
    hist, path, table, pick = reference(tag, start, n_paths, ess_fraction)
    assert min(hist["gaps"], default=np.inf) >= GAP and min(hist["margins"], default=np.inf) >= BOUNDARY and pick >= MARGIN      # (the conditions, where they are used)
    assert got["trajectory"].shape == (1, int(q.n_pts), int(q.dim_d)) and got["slots"].shape == (1, hist["ess"].size + 1)
    assert got["slots"].dtype == np.int32 and np.all(np.isfinite(got["trajectory"]))
    _identities(got, q, ref)
    _against_restatement(got, hist, path, table, label=label)
    if n_paths == 1:
        assert np.array_equal(got["trajectory"][0], ref), label
    if ess_fraction == 0.0:
        flt = ctx.particle_filter(n_paths, SEED, **args)
        assert np.array_equal(got["state"][0, 1:], flt["state"][0, 1:]) and np.array_equal(got["log_w"][0, 1:], flt["log_w"][0, 1:]), label
        assert not got["resampled"].any()
    again = ctx.particle_conditional(ref, n_paths, SEED, history=True, **args)
    assert _same(again, got), label
    bare = ctx.particle_conditional(ref, n_paths, SEED, **args)
    assert bare["ancestors"] is None and np.array_equal(bare["trajectory"], got["trajectory"]) and np.array_equal(bare["slots"], got["slots"])


@pytest.mark.parametrize("d", TIGHT)
def test_tight_lorenz96_clouds(d):
    """Lorenz-96 where ancestor sampling decides (test_particle_gibbs_cpu.test_tight_clouds_react_to_the_transition_term): the ancestors
    of the pinned slot are the restatement's, entry for entry, and not all 0"""
    q, x = tight_case(d)
    hist, path, table, pick = tight_reference(d)
    assert min(hist["gaps"]) >= GAP and min(hist["margins"]) >= BOUNDARY and pick >= MARGIN
    ref = tight_reference_path(d)
    ctx = gpu_context(q)
    got = ctx.particle_conditional(ref, TIGHT_PARTICLES, SEED, ess_fraction=1.0, x=x, prior=_prior(q), history=True)
    ctx.close()
    _identities(got, q, ref)
    _against_restatement(got, hist, path, table, label=f"tight L96 D={d}")
    c = hist["ess"].size
    assert np.any(got["ancestors"][0, :c, 0][hist["resampled"].astype(bool)] != 0)


@pytest.mark.parametrize("model,d", [("L96", 12), ("L63", 3)])
def test_batch_equals_its_single_runs(model, d):
    """B = 3 with own observation times and counts, theta, Sigma, R and H: row k is the restatement of index k, and bit for bit what the
    problem returns beside two other neighbours"""
    runs = {}
    for first in (20, 50):
        probs, xs = batch_case(model, d, first)
        prior = (np.stack([np.asarray(q.mu0, dtype=float) for q in probs]), np.stack([np.asarray(q.tau0, dtype=float) for q in probs]))
        ctx = _batch_context(model, d, probs)
        args = dict(ess_fraction=0.5, x=xs, prior=prior)
        want = batch_reference(model, d, first)
        refs = np.stack([w[0] for w in want])
        runs[first] = (ctx.particle_conditional(refs, 40, SEED_BATCH, history=True, **args), refs)
        ctx.close()
        for k, q in enumerate(probs):
            label = f"{model} batch {first} problem {k}"
            _, hist, path, table, pick = want[k]
            assert min(hist["gaps"], default=np.inf) >= GAP and min(hist["margins"], default=np.inf) >= BOUNDARY and pick >= MARGIN, label
            _against_restatement(runs[first][0], hist, path, table, k=k, label=label)
            _identities(runs[first][0], q, refs[k], k=k)
    a, b = runs[20], runs[50]
    assert np.array_equal(a[1][2], b[1][2])      # (the last problem is the same in both batches, and so is its reference)
    for key, val in a[0].items():
        assert np.array_equal(val[2], b[0][key][2], equal_nan=True), key


def test_neighbours_are_unchanged(contexts):      # noqa: F811
    """particle_filter, particle_paths and particle_backward_paths return the same bits before and after a conditional run"""
    for tag in ("l63_euler_p", "l96d17_rk4_p"):
        q, x, _ = case(tag)
        ctx = _ctx(contexts, tag)
        args = dict(ess_fraction=0.5, x=x, prior=_prior(q))
        before = (ctx.particle_filter(65, SEED, history=True, **args), ctx.particle_paths(65, SEED, 5, **args), ctx.particle_backward_paths(65, SEED, 5, **args))
        ctx.particle_conditional(reference_path(tag, "drawn"), 65, SEED, **args)
        after = (ctx.particle_filter(65, SEED, history=True, **args), ctx.particle_paths(65, SEED, 5, **args), ctx.particle_backward_paths(65, SEED, 5, **args))
        assert all(_same(u, v) for u, v in zip(before, after)), tag


def test_errors():
    """the refusals of particle_paths and a null reference; the context stays usable afterwards"""
    from test_problem_batch import _context, _datasets
    base, probs, xs = _datasets("L96", "euler", 0.5, 12, 3, False)
    ctx = _context(base, probs, 3, 0, obs_t=False)
    mu, tau = np.ones((3, 12)), np.stack([0.5 * np.eye(12)] * 3)
    refs = ctx.particle_paths(5, 2, 1, x=xs, prior=(mu, tau))["paths"][:, 0]
    usable = lambda: ctx.particle_conditional(refs, 5, 1, x=xs, prior=(mu, tau))       # noqa: E731
    with pytest.raises(RuntimeError, match="no cached state"):
        ctx.particle_conditional(refs, 5, 1)
    want = usable()
    with pytest.raises(ValueError):
        ctx.particle_conditional(refs, 0, 1, x=xs)
    with pytest.raises(ValueError, match="ess_fraction"):
        ctx.particle_conditional(refs, 5, 1, ess_fraction=1.5, x=xs)
    with pytest.raises(ValueError, match="null argument"):
        ctx.particle_conditional(None, 5, 1, x=xs)
    with pytest.raises(ValueError, match="ref has"):
        ctx.particle_conditional(refs[:, :-1], 5, 1, x=xs)
    assert _same(usable(), want)
    dense = np.stack([np.reshape(q.sigma, (12, 12)) + 0.1 * (np.ones((12, 12)) - np.eye(12)) * (k == 1) for k, q in enumerate(probs)])
    ctx.set_problem_params(sigma=dense)
    with pytest.raises(NotImplementedError, match="dense Sigma"):
        usable()
    ctx.set_problem_params(sigma=np.stack([np.reshape(q.sigma, (12, 12)) for q in probs]))
    assert _same(usable(), want)
    ctx.close()
    ode = va.Context("NONE", "euler", 3, 10, 0.01, sigma=np.eye(3), batch=2)
    with pytest.raises(ValueError):
        ode.particle_conditional(np.zeros((2, 10, 3)), 2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    ode.close()
    bare = va.Context("L63", "euler", 3, 10, 0.01, sigma=np.eye(3), theta=[10.0, 28.0, 2.667], batch=2)
    with pytest.raises(RuntimeError, match="ODE-only"):
        bare.particle_conditional(np.zeros((2, 10, 3)), 2, 1, x=np.zeros((2, 10 * 12)), x0=np.ones((2, 3)))
    bare.close()
    p, x = make_problem("L96", 72, 9)
    big = gpu_context(p)
    with pytest.raises(NotImplementedError):
        big.particle_conditional(np.zeros((9, 72)), 2, 1, x=x)
    assert np.isfinite(big.free_energy(x))
    big.close()


@pytest.mark.parametrize("tag,d", [("ou_euler", 1), ("dw_euler_p", 1), ("l63_rk4_p", 3)])
def test_chain(tag, d):
    """VarGP.particle_gibbs for 5 iterations on the fixtures' own problems and (A_t, b_t): the same seed gives the same chain; the theta
    trace is the host replay of the conditional draws from the returned trajectories; sweep 1 ran on the device at theta_1 (one
    Context.particle_conditional at that theta from trajectory 0 returns trajectory 1); a ProblemBatch of one and member 0 of a batch of
    three give the single VarGP's chain, and a member's chain is the same bits beside other neighbours"""
    z = load_golden(tag)
    x = np.asarray(z["x"], dtype=float)

    def fresh(shift=0.0):      # (the fixture's problem; shift: another prior mean, which the initial term of a drawn start reads)
        p = problem_from_golden(z)
        p["kl0"].mu0 = np.asarray(p["kl0"].mu0, dtype=float) + shift
        return p["vgp"]
    v = fresh()
    theta0 = np.atleast_1d(np.asarray(v.model.theta, dtype=float)).copy()
    prior = (theta0, (20.0 / theta0) ** 2)      # (a short window says little about theta: the prior keeps OU's theta positive, which the model checks)
    one = v.particle_gibbs(33, 5, 5, theta_prior=prior, x=x)
    v.invalidate()
    assert isinstance(one, va.GibbsChain) and one.theta.shape == (6, theta0.size) and len(one) == 5 and np.array_equal(one.kept, np.arange(5))
    assert one.paths.shape == ((5, v.dim_n) if d == 1 else (5, v.dim_n, d)) and np.array_equal(one.theta[0], theta0)
    assert np.all((one.moved >= 0.0) & (one.moved <= 1.0)) and one.moved.max() > 0.0 and np.all(np.isfinite(one.theta))
    # the host replay of the theta trace
    sig = np.asarray(v._inputs()["sigma"], dtype=float).reshape(d, d).diagonal()
    for it in range(5):
        path = one.paths[it].reshape(v.dim_n, d)
        mean, prec = theta_conditional(v.model._model_id, one.theta[it], path, float(v.fwd_ode.dt), sig, prior)
        assert np.array_equal(one.theta[it + 1], theta_draw(mean, prec, 5, it, 0)), it
    # the new theta reached the device: sweep 1 (seed 5 + 1 + 1) at theta_1 from trajectory 0 is trajectory 1; at theta_0 the weights differ
    w = fresh()
    pb = va.ProblemBatch([w])
    args = dict(ess_fraction=0.5, x=pb._stack(x), prior=w._prior())
    ref = one.paths[0].reshape(1, v.dim_n, d)
    at0 = pb._context().particle_conditional(ref, 33, 7, **args)
    w.model.theta = float(one.theta[1, 0]) if theta0.size == 1 else one.theta[1].copy()
    at1 = pb._context().particle_conditional(ref, 33, 7, **args)
    pb.close()
    assert np.array_equal(at1["trajectory"][0], one.paths[1].reshape(v.dim_n, d)) and not np.array_equal(at1["log_w"], at0["log_w"])
    # the same seed, the same chain
    v2 = fresh()
    two = v2.particle_gibbs(33, 5, 5, theta_prior=prior, x=x)
    v2.invalidate()
    assert np.array_equal(two.theta, one.theta) and np.array_equal(two.paths, one.paths) and np.array_equal(two.moved, one.moved)
    # member 0 of a batch of three is the single chain (counter word 0); member 2 is the same bits beside two other neighbours
    runs = []
    for shifts in ((0.0, 0.1, 0.2), (0.3, 0.4, 0.2)):
        pb = va.ProblemBatch([fresh(sh) for sh in shifts], own_parameters=True)
        runs.append(pb.particle_gibbs(33, 5, 5, theta_prior=prior, x=np.stack([x] * 3)))
        pb.close()
    a, b = runs
    assert len(a) == 3 and np.array_equal(a[0].theta, one.theta) and np.array_equal(a[0].paths, one.paths) and np.array_equal(a[0].moved, one.moved)
    assert np.array_equal(a[2].theta, b[2].theta) and np.array_equal(a[2].paths, b[2].paths) and np.array_equal(a[2].moved, b[2].moved)
    assert not np.array_equal(a[2].paths, one.paths)      # (counter word 2, not 0)
    thin = fresh().particle_gibbs(33, 5, 5, burn=1, thin=2, sample_theta=False, x=x)
    assert np.array_equal(thin.kept, [1, 3]) and np.all(thin.theta == theta0[None, :]) and thin.paths.shape[0] == 2
