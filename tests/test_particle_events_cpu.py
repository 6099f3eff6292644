"""
Path events of the particle filter's lineages (vgpa_particle_events): the numpy restatement, its checks against the filter it rides on and
against the lineage paths, the level recipe and the conditions on the cases of tests/test_particle_events.py, the mutants of the
restatement, the longdouble restatement of the two reductions, the record PathEvents and the host-side surface.

The restatement rides on test_particle_filter_cpu.particle_filter_numpy: walk_numpy takes that filter's ancestors and decisions, walks the
states once more with the same operations (particle_ref.visited_states: gathered through the stored ancestors where the filter resampled) and keeps
every visited state x_i(k), the state of slot i as the walk arrives at k, before a resampling decision at k.  The walk is asserted bit-equal
to the filter's (its clouds at every observation, its final state).  event_rows then carries the row (X, T, N) of
    g_j(x) = s_j (x_j - c_j)   (one subtraction, an exact change of sign; in the event iff g > 0)
per slot along those states, gathering at a resampling, as vgpa_hip.h states it.

Levels.  Per case and component the level is the midpoint of a gap between consecutive sorted visited values inside the component's 20-80 %
quantile range: the widest gap whose midpoint splits the final lineages (some were in the event, some never) where there is one that keeps
the margin below; where that range has none, such a gap anywhere in the component's range; else the widest gap of the 20-80 % range.  (The
plain widest gap leaves collapsed clouds without a component that splits: their lineages share most of their path, and the widest gap in
the middle of the range is crossed by all of them.)  Sides alternate +1 / -1 over the components.
The margin: min |g_j(x)| over all visited states >= 1e-7 max(1, |c_j|), far above the 1e-12 by which device and numpy states differ, so
that the device's rows must be the restatement's exactly.  Under that margin g is never 0, so `>=` for `>` cannot change a row of these
cases: that mutant is held against the same cases with the level of component 0 moved onto a visited state.
"""
import functools
import inspect
import os
import re
import types

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import PathEvents
from conftest import ROOT
from particle_ref import visited_states
from test_particle_filter_cpu import (FRACTIONS, PLACEMENTS, QUIET, SEED, SEED_BATCH, _given, batch_case, case, particle_filter_numpy, placement_case)
from test_particle_paths_cpu import rewalk_numpy, trace_slots
from test_path_weights_cpu import TAGS

EVENT_MARGIN = 1e-7
SIZES = (1, 17, 65, 300)
MUTANTS = ("ge", "no_start", "sentinel", "no_gather", "no_side", "t_max")      # (and "other_level", which needs a batch)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def walk_numpy(problem, x, x0, n, seed, ess_fraction, index=0):
    """The filter of particle_filter_numpy and, from its ancestors, every visited state.  Returns the filter's dict plus visited (Np, n, D),
    gathers: {k: ancestors} for the grid indices k at which the cloud was resampled, n_pts."""
    flt = dict(particle_filter_numpy(problem, x, x0, n, seed, ess_fraction, index=index))
    obs_t = flt["obs_t"]
    gathers = {int(t): flt["ancestors"][j] for j, t in enumerate(obs_t) if flt["resampled"][j]}
    visited, state = visited_states(problem, x, x0, seed, n, gathers, index)
    # the walk is the filter's, bit for bit: its clouds are the visited states at the observations, its final particles the last ones
    for j, t in enumerate(obs_t):
        assert np.array_equal(visited[int(t)], flt["clouds"][j]), ("cloud", j)
    assert np.array_equal(state, flt["state"])
    flt.update(visited=visited, gathers=gathers, n_pts=int(problem.n_pts))
    return flt


def event_rows(walk, levels, side, mutant=None, other_levels=None):
    """rows (n, 3, D) = (X, T, N) of the walk's slots, as vgpa_hip.h states them.  mutant: one deliberate mistake (MUTANTS; "other_level"
    takes other_levels, another problem's)."""
    visited, gathers, n_pts = walk["visited"], walk["gathers"], walk["n_pts"]
    c = np.asarray(other_levels if mutant == "other_level" else levels, dtype=float).reshape(1, -1)
    s = np.ones_like(c) if mutant == "no_side" else np.asarray(side, dtype=float).reshape(1, -1)
    never = n_pts - 1 if mutant == "sentinel" else n_pts
    inside = (lambda g: g >= 0.0) if mutant == "ge" else (lambda g: g > 0.0)
    g = s * (visited[0] - c)
    ins = inside(g)
    big, first, count = g, np.where(ins, 0, never), ins.astype(np.int64)
    if mutant == "no_start":
        big, first, count = np.full_like(g, -np.inf), np.full(g.shape, never), np.zeros(g.shape, dtype=np.int64)
    for k in range(n_pts):
        if k > 0:
            g = s * (visited[k] - c)
            ins = inside(g)
            big = np.maximum(big, g)
            first = np.where(ins, np.maximum(first, k) if mutant == "t_max" else np.minimum(first, k), first)
            count = count + ins
        if k in gathers and mutant != "no_gather":
            big, first, count = big[gathers[k]], first[gathers[k]], count[gathers[k]]
    return np.stack((big, first.astype(float), count.astype(float)), axis=1)


def events_of_paths(paths, levels, side):
    """rows (K, 3, D) of whole trajectories paths (K, Np, D): the definition, evaluated on each path alone"""
    paths = np.asarray(paths, dtype=float)
    n_pts = paths.shape[1]
    g = np.asarray(side, dtype=float).reshape(1, 1, -1) * (paths - np.asarray(levels, dtype=float).reshape(1, 1, -1))
    ins = g > 0.0
    first = np.where(ins.any(axis=1), ins.argmax(axis=1), n_pts)
    return np.stack((g.max(axis=1), first.astype(float), ins.sum(axis=1).astype(float)), axis=1)


def lineage_paths(problem, x, x0, seed, walk, index=0):
    """(n, Np, D): the lineage path of every final slot, by trace_slots + rewalk_numpy of test_particle_paths_cpu"""
    n = walk["state"].shape[0]
    return rewalk_numpy(problem, x, x0, seed, trace_slots(np.arange(n), walk["ancestors"], walk["resampled"]), index=index)


def sides_for(d):
    return np.where(np.arange(d) % 2 == 0, 1, -1).astype(np.int32)


def levels_for(walk, paths):
    """(D,): the recipe of the module docstring, from the visited states and the lineage paths of the final slots"""
    visited = walk["visited"].reshape(-1, walk["visited"].shape[-1])
    side = sides_for(visited.shape[1])
    out = np.empty(visited.shape[1])
    for j in range(visited.shape[1]):
        every = np.unique(visited[:, j])
        reach = paths[:, :, j].max(axis=1) if side[j] > 0 else paths[:, :, j].min(axis=1)      # how far each final lineage went

        def gaps_of(lo, hi):
            """(midpoints, half widths) of the gaps inside the quantile range, widest first"""
            v = every[(every >= np.quantile(every, lo)) & (every <= np.quantile(every, hi))]
            assert v.size >= 2, (j, v.size)
            order = np.argsort(-np.diff(v), kind="stable")
            return (0.5 * (v[:-1] + v[1:]))[order], (0.5 * np.diff(v))[order]

        def splitting(mids, half):
            for c, h in zip(mids, half):
                if h < EVENT_MARGIN * max(1.0, abs(c)):
                    return None
                crossed = reach > c if side[j] > 0 else reach < c
                if crossed.any() and not crossed.all():
                    return c
            return None

        middle = gaps_of(0.2, 0.8)
        found = splitting(*middle)
        if found is None:      # (the whole range only where the middle of it has no gap that splits)
            found = splitting(*gaps_of(0.0, 1.0))
        out[j] = middle[0][0] if found is None else found
    return out


def margin_of(walk, levels):
    """min over components of min |g_j(x)| / max(1, |c_j|) over all visited states"""
    c = np.asarray(levels, dtype=float).reshape(1, 1, -1)
    return float(np.min(np.min(np.abs(walk["visited"] - c), axis=(0, 1)) / np.maximum(1.0, np.abs(c.ravel()))))


def reductions_longdouble(lw, rows, n_pts, stride):
    """(mean (3, D), cdf (n_keep, D)) from given rows and log-weights in longdouble: W_i = w_i / sum w, w_i = exp(lw_i - max lw);
    mean = sum_i W_i row_i; cdf[k'] = sum_i W_i 1[T_i <= k' stride]"""
    lw, rows = np.asarray(lw, dtype=np.longdouble).ravel(), np.asarray(rows, dtype=np.longdouble)
    w = np.exp(lw - lw.max())
    w = w / w.sum()
    kept = np.arange((n_pts - 1) // stride + 1) * stride
    cdf = np.einsum("i,ikd->kd", w, (rows[:, 1][:, None, :] <= kept[None, :, None]).astype(np.longdouble))
    return np.tensordot(w, rows, axes=(0, 0)), cdf


def particle_events_numpy(problem, x, x0, n, seed, ess_fraction, levels, side, stride=1, index=0):
    """One problem's events with counter word `index`: the filter's dict (lw, state, ess, resampled, margins, ...) plus rows (n, 3, D), mean
    (3, D), cdf (n_keep, D) (the reductions in longdouble)."""
    walk = walk_numpy(problem, x, x0, n, seed, ess_fraction, index=index)
    rows = event_rows(walk, levels, side)
    mean, cdf = reductions_longdouble(walk["lw"], rows, walk["n_pts"], stride)
    walk.update(rows=rows, mean=mean, cdf=cdf, levels=np.asarray(levels, dtype=float), side=np.asarray(side))
    return walk


# ---- the cases of the GPU tests, each computed once per process (read-only) --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(problem_key):
    kind = problem_key[0]
    if kind == "grid":
        _, tag, start, n, frac = problem_key
        q, x, x0 = case(tag)
        return q, x, (x0 if start == "given" else None), n, SEED, frac, 0
    if kind == "placement":
        _, model, d, obs_at, given = problem_key
        q, x = placement_case(model, d, obs_at)
        return q, x, (_given(q) if given else None), 17, SEED, 1.0, 0
    _, model, d, first, k = problem_key
    probs, xs = batch_case(model, d, first)
    return probs[k], xs[k], None, 40, SEED_BATCH, 0.5, k


@functools.lru_cache(maxsize=None)
def reference(problem_key):
    """the restatement of one GPU case with the levels and sides of the recipe: ("grid", tag, start, n, ess_fraction),
    ("placement", model, d, obs_at, given) or ("batch", model, d, first, k)"""
    q, x, x0, n, seed, frac, index = _built(problem_key)
    walk = walk_numpy(q, x, x0, n, seed, frac, index=index)
    paths = lineage_paths(q, x, x0, seed, walk, index=index)
    levels, side = levels_for(walk, paths), sides_for(int(q.dim_d))
    rows = event_rows(walk, levels, side)
    walk.update(rows=rows, levels=levels, side=side, paths=paths)
    return walk


def family(problem_key):
    return problem_key[0] if problem_key[0] != "grid" else ("quiet" if problem_key[1] in QUIET else "fixtures")


def gpu_cases():
    keys = [("grid", t, s, n, f) for t in TAGS + QUIET for s in (("given",) if t in QUIET else ("given", "drawn")) for n in SIZES for f in FRACTIONS]
    keys += [("grid", t, s, 17, 0.0) for t in TAGS for s in ("given", "drawn")]
    keys += [("placement", m, d, o, g) for m, d in (("L96", 12), ("L63", 3)) for o in PLACEMENTS for g in (False, True)]
    keys += [("batch", m, d, first, k) for m, d in (("L96", 12), ("L63", 3)) for first in (20, 50) for k in range(3)]
    return keys


# a few of every family for the checks that cost a second walk per mutant
SAMPLE = [("grid", "ou_euler", "drawn", 65, 0.5), ("grid", "l63_euler_p", "given", 17, 1.0), ("grid", "l96d12_euler_p", "drawn", 65, 0.5),
          ("grid", "quiet_l96d12", "given", 65, 0.5), ("grid", "quiet_l96d17", "given", 300, 0.5),
          ("placement", "L96", 12, PLACEMENTS[0], False), ("placement", "L63", 3, PLACEMENTS[2], True),
          ("batch", "L96", 12, 20, 0), ("batch", "L63", 3, 20, 1), ("batch", "L96", 12, 50, 2)]


# ---- the restatement against the filter and the lineage paths ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SAMPLE, ids=str)
def test_same_walk_as_the_filter(key):
    q, x, x0, n, seed, frac, index = _built(key)
    ref = reference(key)      # (walk_numpy asserts the clouds and the final state bit for bit)
    flt = particle_filter_numpy(q, x, x0, n, seed, frac, index=index)
    for name in ("lw", "state", "ess", "resampled", "ancestors"):
        assert np.array_equal(ref[name], flt[name]), (key, name)
    assert ref["margins"] == flt["margins"]
    full = particle_events_numpy(q, x, x0, n, seed, frac, ref["levels"], ref["side"], stride=3, index=index)      # (the one-call form of the same)
    assert np.array_equal(full["rows"], ref["rows"]) and np.array_equal(full["lw"], flt["lw"])
    assert full["mean"].shape == ref["rows"].shape[1:] and full["cdf"].shape == ((ref["n_pts"] - 1) // 3 + 1, ref["rows"].shape[2])


@pytest.mark.parametrize("key", gpu_cases(), ids=str)
def test_rows_are_the_events_of_the_lineage_paths(key):
    """exactly: the carried rows are the definition evaluated on the path of the lineage that ends in each final slot"""
    ref = reference(key)
    assert np.array_equal(ref["paths"][:, -1], ref["state"])
    assert np.array_equal(ref["rows"], events_of_paths(ref["paths"], ref["levels"], ref["side"])), key


def test_margin_and_the_conditions_on_the_cases():
    """conditions on the cases, not measurements of the device: the margin for every case the GPU file runs; every case with more than one
    particle has a component that some final lineages crossed and some did not -- but the two in which no level whatever can do that, which
    are named --; some row has T = 0, some keeps the sentinel; in the quiet
    cases rows are both copied and carried"""
    worst, seen_zero, seen_never, quiet_kinds, no_level_splits = {}, False, False, set(), []
    for key in gpu_cases():
        ref = reference(key)
        m = margin_of(ref, ref["levels"])
        worst[family(key)] = min(worst.get(family(key), np.inf), m)
        assert m >= EVENT_MARGIN, (key, m)
        t = ref["rows"][:, 1]
        if ref["state"].shape[0] > 1:
            # (no level at all can split lineages that went equally far in every component: one survivor at the last resampling, at index
            # Np - 2, and no new extreme in the one step behind it)
            reach = np.where(ref["side"] > 0, ref["paths"].max(axis=1), ref["paths"].min(axis=1))
            if all(np.unique(reach[:, j]).size == 1 for j in range(reach.shape[1])):
                no_level_splits.append(key)
            else:
                share = np.mean(t < ref["n_pts"], axis=0)
                assert np.any((share > 0.0) & (share < 1.0)), (key, share)
        seen_zero |= bool(np.any(t == 0.0))
        seen_never |= bool(np.any(t == ref["n_pts"]))
        if family(key) == "quiet" and key[3] >= 65:
            quiet_kinds |= set(ref["resampled"][:-1].tolist())
    print("smallest event margin per family:", worst)
    assert set(worst) == {"fixtures", "quiet", "placement", "batch"}
    assert seen_zero and seen_never and quiet_kinds == {0, 1}
    assert no_level_splits == [("placement", "L63", 3, PLACEMENTS[2], False), ("placement", "L63", 3, PLACEMENTS[2], True)], no_level_splits


def test_mutants_change_a_row_in_every_family():
    """every deliberate mistake changes at least one row entry in every family of cases.  `>=` for `>` is held against the cases with the
    level of component 0 moved onto a state some final lineage visits (the margin excludes g = 0 otherwise); another problem's level needs a
    batch and is held against that family"""
    hit = {m: set() for m in MUTANTS + ("other_level",)}
    for key in gpu_cases():
        ref = reference(key)
        fam = family(key)
        for m in MUTANTS:
            if fam in hit[m]:
                continue
            levels = ref["levels"].copy()
            if m == "ge":
                levels[0] = ref["paths"][0, ref["n_pts"] // 2, 0]
                assert np.array_equal(event_rows(ref, levels, ref["side"]), events_of_paths(ref["paths"], levels, ref["side"]))
            if not np.array_equal(event_rows(ref, levels, ref["side"], mutant=m), event_rows(ref, levels, ref["side"])):
                hit[m].add(fam)
        if fam == "batch" and "batch" not in hit["other_level"]:
            other = reference(key[:4] + ((key[4] + 1) % 3,))["levels"]
            if not np.array_equal(event_rows(ref, ref["levels"], ref["side"], mutant="other_level", other_levels=other), ref["rows"]):
                hit["other_level"].add("batch")
    print({m: sorted(f) for m, f in hit.items()})
    for m in MUTANTS:
        assert hit[m] == {"fixtures", "quiet", "placement", "batch"}, (m, hit[m])
    assert hit["other_level"] == {"batch"}


# ---- the reductions --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SAMPLE, ids=str)
def test_reductions(key):
    ref = reference(key)
    n_pts = ref["n_pts"]
    w = np.exp(ref["lw"] - ref["lw"].max())
    w = w / w.sum()
    for stride in (1, 3, 7):
        mean, cdf = reductions_longdouble(ref["lw"], ref["rows"], n_pts, stride)
        assert cdf.shape == ((n_pts - 1) // stride + 1, ref["rows"].shape[2]) and np.all(np.diff(cdf, axis=0) >= 0)
        assert np.max(np.abs(mean - np.tensordot(w, ref["rows"], axes=(0, 0))) / np.maximum(np.abs(mean), 1e-300)) <= 1e-13
        assert np.array_equal(cdf[0].astype(float) > 0, np.any(ref["rows"][:, 1] == 0, axis=0) & (cdf[0] > 0))
        if (n_pts - 1) % stride == 0:
            crossed = np.tensordot(w, (ref["rows"][:, 1] < n_pts).astype(float), axes=(0, 0))
            assert np.max(np.abs(cdf[-1].astype(float) - crossed)) <= 1e-13
        full = reductions_longdouble(ref["lw"], ref["rows"], n_pts, 1)[1]
        assert np.array_equal(cdf, full[::stride])
    # E[N] counts what the cdf's increments place: N >= 1 exactly where T is no sentinel
    assert np.array_equal(ref["rows"][:, 2] >= 1, ref["rows"][:, 1] < n_pts)
    assert np.all(ref["rows"][:, 2] <= n_pts - ref["rows"][:, 1])


# ---- the record and the surface --------------------------------------------------------------------------------------------------------------
def test_record_on_a_hand_made_table():
    # two components, five grid indices, four particles of equal weight; component 1 looks below its level
    rows = np.array([[[0.5, -0.2], [0.0, 5.0], [3.0, 0.0]], [[1.5, 0.4], [2.0, 4.0], [2.0, 1.0]], [[-0.1, 0.3], [5.0, 1.0], [0.0, 2.0]],
                     [[0.2, -0.3], [4.0, 5.0], [1.0, 0.0]]])
    lw = np.zeros(4)
    mean, cdf = reductions_longdouble(lw, rows, 5, 1)
    rec = PathEvents(lw, mean.astype(float), cdf.astype(float), [1.0, -1.0], [1, -1], 1, 5, 0.1, [3.0], [1], rows)
    assert len(rec) == 4 and rec.dim_d == 2 and np.array_equal(rec.grid, np.arange(5))
    assert np.allclose(rec.prob_crossed, [0.75, 0.5]) and np.allclose(rec.cdf[:, 0], [0.25, 0.25, 0.5, 0.5, 0.75])
    assert np.allclose(rec.occupation_time, 0.1 * np.array([1.5, 0.75]))
    assert np.allclose(rec.mean_extreme, [1.0 + 0.525, -1.0 - 0.05])
    assert np.array_equal(rec.first_passage_quantile(0.5), [2.0, 4.0]) and np.isnan(rec.first_passage_quantile(0.9)).all()
    assert np.allclose(rec.extreme_quantile(0.5), [1.0 + 0.2, -1.0 + 0.2]) and np.allclose(rec.extreme_quantile(1.0), [2.5, -1.4])
    grid, dist = rec.first_passage_cdf()
    assert np.array_equal(grid, rec.grid) and np.array_equal(dist, rec.cdf)
    # a stride that does not divide Np - 1: the last kept index is 3, the crossing at 4 is in the rows alone
    m3, c3 = reductions_longdouble(lw, rows, 5, 3)
    coarse = PathEvents(lw, m3.astype(float), c3.astype(float), [1.0, -1.0], [1, -1], 3, 5, 0.1, rows=rows)
    assert np.array_equal(coarse.grid, [0, 3]) and np.allclose(coarse.prob_crossed, [0.75, 0.5]) and np.allclose(coarse.cdf[-1], [0.5, 0.25])
    with pytest.raises(ValueError, match="rows"):
        PathEvents(lw, m3.astype(float), c3.astype(float), [1.0, -1.0], [1, -1], 3, 5, 0.1).prob_crossed
    with pytest.raises(ValueError, match="rows"):
        PathEvents(lw, mean.astype(float), cdf.astype(float), 1.0, 1, 1, 5, 0.1).extreme_quantile(0.5)
    for bad in (lambda: PathEvents([], mean, cdf, 1.0, 1, 1, 5, 0.1), lambda: PathEvents(lw, mean[:2], cdf, 1.0, 1, 1, 5, 0.1),
                lambda: PathEvents(lw, mean, cdf[:3], 1.0, 1, 1, 5, 0.1), lambda: PathEvents(lw, mean, cdf, 1.0, 2, 1, 5, 0.1),
                lambda: PathEvents(lw, mean, cdf, 1.0, 1, 0, 5, 0.1), lambda: PathEvents(lw, mean, cdf, 1.0, 1, 1, 5, 0.1, rows=rows[:3]),
                lambda: PathEvents(lw, mean, cdf, 1.0, 1, 1, 5, 0.1, [1.0], [])):
        with pytest.raises(ValueError):
            bad()


def test_symbol_and_prototype():
    assert "vgpa_particle_events" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header) and _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_events\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, uint64_t seed, "
                    "double ess_fraction, const double* prior_mu_or_null, const double* prior_tau_or_null, const double* levels, "
                    "const int32_t* sides, double* logw, double* state, double* rows_or_null, double* mean_or_null, double* cdf_or_null, "
                    "double* ess_or_null, int32_t* resampled_or_null")


def test_python_surface():
    for owner, params in [(va.Context, ["n_paths", "seed", "levels", "side", "stride", "ess_fraction", "x", "x0", "prior", "per_particle"]),
                          (va.VarGP, ["n_paths", "seed", "levels", "side", "stride", "ess_fraction", "x", "x0", "per_particle"]),
                          (va.ProblemBatch, ["n_paths", "seed", "levels", "side", "stride", "ess_fraction", "x", "x0", "per_particle"])]:
        fn = getattr(owner, "particle_events", None)
        assert callable(fn), owner.__name__
        sig = inspect.signature(fn).parameters
        assert list(sig)[1:] == params, owner.__name__
        assert sig["side"].default == 1 and sig["stride"].default == 1 and sig["ess_fraction"].default == 0.5 and sig["per_particle"].default is False
    assert va.PathEvents is PathEvents and "PathEvents" in va.__all__
    for name in ("first_passage_cdf", "first_passage_quantile", "extreme_quantile", "log_evidence", "weights"):
        assert callable(getattr(PathEvents, name))
    for name in ("prob_crossed", "occupation_time", "mean_extreme"):
        assert isinstance(getattr(PathEvents, name), property)


def test_argument_checks_of_the_python_layer():
    """levels and side on their way to the C ABI (no device needed: the check is the context's own method on its B and D)"""
    lay = functools.partial(va.Context._event_inputs, types.SimpleNamespace(B=2, D=3))
    lev, sd = lay(0.5, 1)
    assert lev.shape == (2, 3) and lev.dtype == np.float64 and lev.flags.c_contiguous and np.all(lev == 0.5)
    assert sd.shape == (2, 3) and sd.dtype == np.int32 and sd.flags.c_contiguous and np.all(sd == 1)
    lev, sd = lay([1.0, 2.0, 3.0], [1, -1, 1])
    assert np.array_equal(lev, [[1.0, 2.0, 3.0]] * 2) and np.array_equal(sd, [[1, -1, 1]] * 2)
    lev, sd = lay(np.arange(6.0).reshape(2, 3), -np.ones((2, 3)))
    assert np.array_equal(lev, np.arange(6.0).reshape(2, 3)) and np.all(sd == -1)
    for bad in (np.nan, np.inf, [1.0, -np.inf, 0.0]):
        with pytest.raises(ValueError, match="finite"):
            lay(bad, 1)
    for bad in (0, 2, [1, -1, 0], 0.5):
        with pytest.raises(ValueError, match=r"\+1 or -1"):
            lay(0.0, bad)
    with pytest.raises(ValueError, match="levels has"):
        lay([1.0, 2.0], 1)
    with pytest.raises(ValueError, match="side has"):
        lay(0.0, [1, -1])
