"""
The pinned slot's ancestor draw where it decides, on the GPU (vgpa_particle_conditional, vgpa_particle_backward_paths; DESIGN.md s.4.18
"Tests").  Every case, condition, floor and mutant is test_particle_ancestor_cpu's, asserted there without a device; this module only
runs the device and compares.

  A  the decisive cases (OU, DW, L63, L96 at D = 5, 17, 64; 2 .. 300 particles; a batch of three): `resampled`, `ancestors` and `slots` of
     particle_conditional(history=True) entry for entry against the restatement, the four bit identities, log_w, state and trajectory at
     test_particle_gibbs.py's yardstick |got - want| <= 1e-9 (scale + tiny); the same problems through particle_backward_paths, table exact.
     Every mutant of test_particle_ancestor_cpu.MUTANTS changes an entry of these tables.
  B  observation placement (index 0, adjacent indices, the last index) through the conditional filter.
  C  the pinned slot's log-weight without resampling against the longdouble start, path and observation terms of the reference, held to
     err_k <= 32 max(err_o, floor) (test_particle_rounding_cpu's measure).
Every grid has 41 points, every run at most 300 particles, every batch three problems.
"""
import numpy as np
import pytest

import vgpa_amd as va
from test_gpu_edge_cases import gpu_context
from test_particle_ancestor_cpu import (BACKWARD_DRAWS, BACKWARD_GAP, BACKWARD_PARTICLES, BATCH_MODELS, BATCH_PARTICLES, BOUNDARY, DECISIVE, GAP, MARGIN, N_PTS,
                                        PLACED_PARTICLES, SEED, WEIGHT_MODELS, WEIGHT_PARTICLES, WEIGHT_REFERENCES, WEIGHT_SEED, _given,
                                        batch_decisive, batch_decisive_reference, case_seed, check_pinned_weight, decisive_backward,
                                        decisive_case, decisive_reference, decisive_reference_path, decisive_runs, pick_slots, pinned_ancestors,
                                        placement_case, placement_reference, placement_runs, weight_case, weight_references)
from test_particle_backward import _against_itself, _against_numpy
from test_particle_filter import _prior
from test_particle_gibbs import _against_restatement, _identities

pytestmark = pytest.mark.gpu
WORST = {}                 # (kernel family, quantity) -> the worst ratio err_k / max(err_o, floor) of this process's run


@pytest.fixture(scope="module")
def contexts():
    """one context per decisive case, closed behind the last test of the module"""
    cache = {}
    yield cache
    for ctx in cache.values():
        ctx.close()


def _ctx(cache, model, d):
    if (model, d) not in cache:
        cache[model, d] = gpu_context(decisive_case(model, d)[0])
    return cache[model, d]


def batch_context(probs):
    """B problems with their own theta, Sigma, start moments, observation counts, times, values and noise; problem 0 has the most observations"""
    q0, nb = probs[0], len(probs)
    d = int(q0.dim_d)
    square = lambda v: np.reshape(np.asarray(v, dtype=float), (d, d))      # noqa: E731
    counts = [int(np.asarray(q.obs_t).size) for q in probs]
    assert counts[0] == max(counts)
    obs_t, obs_y = np.full((nb, counts[0]), -1, dtype=np.int64), np.full((nb, counts[0], d), np.nan)
    for k, q in enumerate(probs):
        obs_t[k, :counts[k]], obs_y[k, :counts[k]] = np.asarray(q.obs_t), np.reshape(np.asarray(q.obs_y, dtype=float), (counts[k], d))
    ctx = va.Context(q0.model, "euler", d, int(q0.n_pts), float(q0.dt), sigma=square(q0.sigma), theta=np.atleast_1d(q0.theta), m0=np.atleast_1d(q0.m0),
                     s0=square(q0.s0), obs_t=q0.obs_t, obs_y=q0.obs_y, obs_noise=square(q0.obs_noise),
                     obs_h=None if d == 1 else square(q0.obs_h), batch=nb)
    ctx.set_problem_obs_model(n_obs=counts, obs_noise=np.stack([square(q.obs_noise) for q in probs]),
                              obs_h=None if d == 1 else np.stack([square(q.obs_h) for q in probs]))
    ctx.set_problem_data(obs_t=obs_t, obs_y=obs_y, m0=np.stack([np.atleast_1d(np.asarray(q.m0, dtype=float)) for q in probs]),
                         s0=np.stack([square(q.s0) for q in probs]))
    ctx.set_problem_params(theta=np.stack([np.atleast_1d(np.asarray(q.theta, dtype=float)) for q in probs]),
                           sigma=np.stack([square(q.sigma) for q in probs]))
    return ctx


def _priors(probs):
    d = int(probs[0].dim_d)
    return (np.stack([np.reshape(np.asarray(q.mu0, dtype=float), d) for q in probs]),
            np.stack([np.reshape(np.asarray(q.tau0, dtype=float), (d, d)) for q in probs]))


# ---- A: the decisive cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d,n_paths", decisive_runs())
def test_decisive_conditional(contexts, model, d, n_paths):
    """k_sample_small<1 | 3, Conditional> and k_sample_mfma<16 | 32 | 64, Conditional> between the cuts; k_pf_cresample with two candidates, a
    full wave, one more, one full pass, one more and two partial passes: the pinned slot's ancestors are the restatement's, entry for entry"""
    q, x = decisive_case(model, d)
    ref, seed = decisive_reference_path(model, d), case_seed(model, d, n_paths)
    hist, path, table, pick = decisive_reference(model, d, n_paths)
    assert min(hist["gaps"]) >= GAP and min(hist["margins"]) >= BOUNDARY and pick >= MARGIN      # (the conditions, where they are used)
    got = _ctx(contexts, model, d).particle_conditional(ref, n_paths, seed, ess_fraction=1.0, x=x, prior=_prior(q), history=True)
    _identities(got, q, ref)
    _against_restatement(got, hist, path, table, label=f"decisive {model} D={d} n={n_paths}")
    c = hist["ess"].size
    assert np.array_equal(got["ancestors"][0, :c, 0][hist["resampled"].astype(bool)], pinned_ancestors(hist))


@pytest.mark.parametrize("model,d", DECISIVE)
def test_decisive_backward(contexts, model, d):
    """k_pf_backward's LDS-tile statement of the transition mean on the same problems: the table is the restatement's, entry for entry"""
    q, x = decisive_case(model, d)
    hist, final, table, gaps = decisive_backward(model, d)
    assert min(float(g.min()) for g in gaps) >= BACKWARD_GAP and min(hist["margins"]) >= MARGIN
    assert pick_slots(hist["lw"], BACKWARD_DRAWS, SEED, N_PTS)[1] >= MARGIN
    ctx = _ctx(contexts, model, d)
    label = f"decisive {model} D={d} backward"
    args = dict(ess_fraction=1.0, x=x, prior=_prior(q))
    flt = ctx.particle_filter(BACKWARD_PARTICLES, SEED, history=True, **args)
    got = ctx.particle_backward_paths(BACKWARD_PARTICLES, SEED, BACKWARD_DRAWS, **args)
    _against_itself(got, flt, np.asarray(q.obs_t, dtype=int).ravel(), label=label)
    assert np.array_equal(got["resampled"][0], hist["resampled"]) and np.array_equal(got["slots"][0, -1], final), label
    assert np.array_equal(got["slots"][0], table), (label, np.argwhere(got["slots"][0] != table)[:4])
    _against_numpy(got, q, x, None, SEED, hist, label=label)


@pytest.mark.parametrize("model,d", BATCH_MODELS)
def test_decisive_batch(model, d):
    """B = 3 in the decisive regime: theta_v, R_stride and n_obs_v of k_pf_cresample; row k is the restatement of counter word k"""
    probs, xs = batch_decisive(model, d)
    want = batch_decisive_reference(model, d)
    refs = np.stack([w[0] for w in want])
    ctx = batch_context(probs)
    got = ctx.particle_conditional(refs, BATCH_PARTICLES, SEED, ess_fraction=1.0, x=xs, prior=_priors(probs), history=True)
    ctx.close()
    for k, q in enumerate(probs):
        label = f"decisive {model} D={d} batch problem {k}"
        _, hist, path, table, pick = want[k]
        assert min(hist["gaps"]) >= GAP and min(hist["margins"]) >= BOUNDARY and pick >= MARGIN, label
        _against_restatement(got, hist, path, table, k=k, label=label)
        _identities(got, q, refs[k], k=k)


# ---- B: observation placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d,obs_at,start", placement_runs(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_placement(model, d, obs_at, start):
    """an observation at grid index 0, adjacent indices (the ref[k + 1] load, k_pf_ref_fill's stretch boundaries) and the last index (never
    resampled) through the conditional filter, with a drawn and a given start"""
    q, x = placement_case(model, d, obs_at)
    x0, ref, hist, path, table, pick = placement_reference(model, d, obs_at, start)
    assert min(hist["gaps"], default=np.inf) >= GAP and min(hist["margins"], default=np.inf) >= BOUNDARY and pick >= MARGIN
    ctx = gpu_context(q)
    got = ctx.particle_conditional(ref, PLACED_PARTICLES, SEED, ess_fraction=1.0, x=x, x0=x0, prior=_prior(q), history=True)
    ctx.close()
    _identities(got, q, ref)
    _against_restatement(got, hist, path, table, label=f"placement {model} D={d} at {obs_at} {start}")
    if obs_at[-1] == int(q.n_pts) - 1:
        assert got["resampled"][0, len(obs_at) - 1] == 0


# ---- C: the pinned weight ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", WEIGHT_MODELS)
def test_pinned_weight(model, d):
    """log_w[:, 0] of particle_conditional(ess_fraction=0) -- k_pf_pin's start term, the implied increments of the conditional walk, the
    observation terms -- against the longdouble terms of the reference itself: B = 3 with own parameters, given and drawn start, a drawn and
    a smooth reference, one particle and 65"""
    probs, xs = weight_case(model, d)
    ctx = batch_context(probs)
    family = ("k_sample_small" if d <= 4 else "k_sample_mfma") + "<Conditional>, k_pf_pin"
    fails = []
    for start in ("given", "drawn"):
        x0 = np.stack([_given(q) for q in probs]) if start == "given" else None
        for kind in WEIGHT_REFERENCES:
            refs = weight_references(model, d, start, kind)
            for n in WEIGHT_PARTICLES:
                got = ctx.particle_conditional(refs, n, WEIGHT_SEED, ess_fraction=0.0, x=xs, x0=x0, prior=_priors(probs))
                assert not got["resampled"].any() and np.array_equal(got["state"][:, 0], refs[:, -1])
                assert n > 1 or np.array_equal(got["trajectory"], refs)
                for k, q in enumerate(probs):
                    fails += check_pinned_weight(WORST, f"{model}{d} {start} {kind} n={n} p={k}", family, q, xs[k], start, refs[k], got["log_w"][k, 0])
    ctx.close()
    assert not fails, fails


def test_print_worst():
    """(last: the worst ratio per family of this run)"""
    for (family, quantity), r in sorted(WORST.items()):
        print(f"WORST {family} / {quantity}: {r:.3f}")
