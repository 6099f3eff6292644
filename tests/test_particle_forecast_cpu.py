"""
The particle forecast (vgpa_particle_forecast): the numpy restatement, its own properties, an exact anchor on a linear chain, the margin
condition of the GPU tests, the record Forecast and the host-side surface.

forecast_numpy is the reference of tests/test_particle_forecast.py: a cloud of n particles with log-weights lw at the absolute grid index
index0, carried for h = 1 .. H by
    x_i <- (x_i + dt f(x_i; theta)) + R_jj xi_j,   xi from the counters (index0 + h, i, problem, .),   R = chol_lower(Sigma dt), Sigma diagonal
(normals and model_drift of test_sample_paths_cpu), the moments sum_i W_i x_i and sum_i W_i x_i^2 at h = 0, stride, ... with
W = w / sum w, w = exp(lw - max lw), and the members walked alone, as the device walks them: member m starts from slot s[m] and draws with
the counter word s[m].  The slots are given or come from pick_slots (test_particle_paths_cpu) with the uniform of grid index index0 + 1.

The device forms the prefix sums of the pick in another association than np.cumsum, so its slots are the restatement's where every
threshold keeps a margin from every prefix sum: test_margin_condition asserts >= MARGIN for every drawn-slot run of the GPU tests.
"""
import functools
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from vgpa_amd.particles import Forecast
from conftest import ROOT
from test_gpu_edge_cases import make_problem
from test_particle_filter_cpu import MARGIN, QUIET, SEED, case
from test_particle_filter_cpu import reference as filter_reference
from test_particle_paths_cpu import pick_slots
from test_path_weights_cpu import TAGS, _sigma_diag
from test_sample_paths_cpu import model_drift, normals

# the shapes of the GPU tests: the one-lane kernels' four models (Lorenz-96 at D = 4 is their circular branch), then the LDS kernel at its
# smallest D (odd: the last pair drops a normal), 12, 17 (odd), 40 and 64 (its largest)
SHAPES = [("OU", 1), ("DW", 1), ("L63", 3), ("L96", 4), ("L96", 5), ("L96", 12), ("L96", 17), ("L96", 40), ("L96", 64)]
SIZES = (1, 17, 65, 300)      # one particle; a partial wave; two / five workgroups above D = 4; two below
# (horizon, stride, index0): nothing to walk, at the last index an int holds; one step from 0; a last step that is not kept; 20 steps up to
# the last index an int holds
STEPS = [(0, 1, 2 ** 31 - 1), (1, 1, 0), (7, 3, 40), (20, 1, 2 ** 31 - 21)]
WEIGHTS = ("equal", "random", "dominant", "wide")
FC_SEED = 11
# (model, D, particles, members, weights) of the GPU tests' drawn slots on a given cloud, at index0 = 40
DRAWN = [(m, d, n, k, w) for m, d in (("OU", 1), ("L63", 3), ("L96", 5), ("L96", 40)) for n, k in ((1, 17), (17, 65), (65, 17), (300, 5))
         for w in ("equal", "random", "wide")] + [("L96", 12, 65, 5, "dominant")]
# (tag, start, particles, members) of the GPU tests' drawn slots behind the filter (ess_fraction 0.5, seed SEED)
BEHIND = [(t, s, n, k) for t in TAGS + QUIET for s in (("given",) if t in QUIET else ("given", "drawn")) for n, k in ((17, 65), (300, 65))]


@functools.lru_cache(maxsize=None)
def shape_problem(model, d):
    """a problem of 41 grid points with distinct diagonal entries of Sigma (read-only)"""
    return make_problem(model, d, 41, method="euler")[0]


@functools.lru_cache(maxsize=None)
def cloud_case(model, d, n, weights, k=0):
    """(cloud (n, D), log_w (n,) or None) of problem k: particles around the model's usual range, and log-weights that are equal, random
    (spread 3), one dominant (the others 40 below) or spanning 300 from the largest to the smallest"""
    rng = np.random.default_rng([d, n, k, WEIGHTS.index(weights)])
    centre = {"OU": 0.0, "DW": 1.0, "L63": 1.0, "L96": 8.0}[model]
    cloud = centre + rng.standard_normal((n, d))
    if weights == "equal":
        return cloud, None
    lw = -7.0 + 3.0 * rng.standard_normal(n)
    if weights == "dominant":
        lw[n // 2] += 40.0
    if weights == "wide":
        lw = -300.0 * rng.permutation(n) / max(n - 1, 1)
    cloud.setflags(write=False)
    lw.setflags(write=False)
    return cloud, lw


def weights_of(log_w, n):
    lw = np.zeros(n) if log_w is None else np.asarray(log_w, dtype=float).ravel()
    w = np.exp(lw - lw.max())
    return w / np.sum(w)


def forecast_numpy(problem, cloud, log_w, index0, horizon, stride, seed, slots, index=0):
    """One problem's forecast with counter word `index`.  slots: (K,) given slots, an int K (drawn from log_w with the uniform of grid
    index index0 + 1) or None (no members).  Returns a dict: moments (h_keep, 2, D), members (K, h_keep, D), slots (K,), state_end (n, D),
    margin (of a drawn pick, else inf)."""
    d, dt = int(problem.dim_d), float(problem.dt)
    fac = np.sqrt(_sigma_diag(problem).diagonal() * dt)      # chol_lower of a diagonal matrix
    theta = np.asarray(problem.theta, dtype=float)
    state = np.array(cloud, dtype=float).reshape(-1, d)
    n = state.shape[0]
    w = weights_of(log_w, n)
    margin = np.inf
    if slots is None:
        slots = np.zeros(0, dtype=np.int64)
    elif np.ndim(slots) == 0:
        slots, margin = pick_slots(np.zeros(n) if log_w is None else log_w, int(slots), seed, index0 + 1, index=index)
    slots = np.asarray(slots, dtype=np.int64)
    h_keep = horizon // stride + 1

    def walk(x, words, weigh):
        kept, mom = np.empty((x.shape[0], h_keep, d)), np.empty((h_keep, 2, d))
        for h in range(horizon + 1):
            if h > 0:
                x = (x + dt * model_drift(problem.model, theta, x)) + fac * normals(seed, index0 + h, words, index, d)
            if h % stride == 0:
                kept[:, h // stride] = x
                if weigh:
                    mom[h // stride] = w @ x, w @ (x * x)
        return x, kept, mom

    end, _, moments = walk(state, np.arange(n), True)
    members = walk(state[slots], slots, False)[1] if slots.size else np.empty((0, h_keep, d))
    return dict(moments=moments, members=members, slots=slots, state_end=end, margin=margin)


class OU:
    model, dim_d, n_pts, dt, theta, sigma = "OU", 1, 41, 0.01, 2.0, 0.5


def test_splitting_property():
    """H steps = H1 steps, then H - H1 from its end state with index0 + H1: the states bit for bit, the kept steps line up"""
    for model, d in SHAPES:
        q = shape_problem(model, d)
        cloud, lw = cloud_case(model, d, 17, "random")
        whole = forecast_numpy(q, cloud, lw, 33, 12, 3, FC_SEED, np.array([5, 16, 0]))
        first = forecast_numpy(q, cloud, lw, 33, 6, 3, FC_SEED, np.array([5, 16, 0]))
        rest = forecast_numpy(q, first["state_end"], lw, 39, 6, 3, FC_SEED, np.array([5, 16, 0]))
        assert np.array_equal(rest["state_end"], whole["state_end"]), (model, d)
        assert np.array_equal(np.concatenate((first["moments"], rest["moments"][1:])), whole["moments"])
        assert np.array_equal(np.concatenate((first["members"], rest["members"][:, 1:]), axis=1), whole["members"])
        assert not np.array_equal(forecast_numpy(q, first["state_end"], lw, 38, 6, 3, FC_SEED, None)["state_end"], whole["state_end"])


def test_a_member_is_its_slot_of_the_cloud():
    """member m, walked alone with the counter word of its slot, is row slots[m] of the whole cloud's walk -- for given slots (out of
    order, repeated) and for drawn ones"""
    for model, d in SHAPES:
        q = shape_problem(model, d)
        cloud, lw = cloud_case(model, d, 17, "random")
        every = forecast_numpy(q, cloud, lw, 40, 7, 1, FC_SEED, np.arange(17))
        assert np.array_equal(every["members"][:, -1], every["state_end"]) and np.array_equal(every["members"][:, 0], cloud)
        for slots in (np.array([16, 0, 5, 5, 11]), 9):
            got = forecast_numpy(q, cloud, lw, 40, 7, 1, FC_SEED, slots)
            assert np.array_equal(got["members"], every["members"][got["slots"]]), (model, d)
        strided = forecast_numpy(q, cloud, lw, 40, 7, 3, FC_SEED, np.arange(17))
        assert strided["members"].shape == (17, 3, d) and np.array_equal(strided["members"], every["members"][:, ::3])
        assert np.array_equal(strided["moments"], every["moments"][::3]) and np.array_equal(strided["state_end"], every["state_end"])


def test_horizon_zero():
    q = shape_problem("L96", 5)
    cloud, lw = cloud_case("L96", 5, 17, "wide")
    got = forecast_numpy(q, cloud, lw, 2 ** 31 - 1, 0, 4, FC_SEED, np.array([3, 3]))
    w = weights_of(lw, 17)
    assert got["moments"].shape == (1, 2, 5) and got["members"].shape == (2, 1, 5)
    assert np.array_equal(got["state_end"], cloud) and np.array_equal(got["members"][:, 0], cloud[[3, 3]])
    assert np.array_equal(got["moments"][0], np.stack((w @ cloud, w @ (cloud * cloud))))
    assert abs(w.sum() - 1.0) < 1e-15 and w.min() < 1e-100 * w.max()


def test_weights_do_not_change_and_are_honoured():
    q = shape_problem("L63", 3)
    cloud, lw = cloud_case("L63", 3, 65, "dominant")
    got = forecast_numpy(q, cloud, lw, 40, 5, 1, FC_SEED, np.array([32]))
    # one dominant weight: the mean is that particle's trajectory up to exp(-40) of the others
    assert np.allclose(got["moments"][:, 0], got["members"][0], rtol=1e-12, atol=1e-12)
    equal = forecast_numpy(q, cloud, None, 40, 5, 1, FC_SEED, None)
    assert np.allclose(equal["moments"][-1, 0], equal["state_end"].mean(axis=0), rtol=1e-13)
    assert np.array_equal(equal["state_end"], got["state_end"])


def test_ou_anchor():
    """4096 equally weighted particles of the OU chain against the closed form of its Euler chain: a = 1 - theta dt,
    mean_h = a^h mean_0, var_h = a^2h var_0 + sigma dt (1 - a^2h) / (1 - a^2), within 5 standard errors"""
    n, hor = 4096, 60
    rng = np.random.default_rng(1)
    cloud = 0.7 + 0.4 * rng.standard_normal((n, 1))
    got = forecast_numpy(OU, cloud, None, 40, hor, 10, 2026, None)
    a = 1.0 - OU.theta * OU.dt
    mean0, var0 = float(cloud.mean()), float(cloud.var())
    for slot, h in enumerate(range(0, hor + 1, 10)):
        mean_h = a ** h * mean0
        var_h = a ** (2 * h) * var0 + OU.sigma * OU.dt * (1.0 - a ** (2 * h)) / (1.0 - a * a)
        m1, m2 = got["moments"][slot, :, 0]
        # the cloud's own mean and variance are exact at h = 0; the noise added since has variance var_h - a^2h var0
        noise = var_h - a ** (2 * h) * var0
        se_mean = np.sqrt(noise / n)
        se_var = np.sqrt(2.0 / n) * var_h
        assert abs(m1 - mean_h) <= 5.0 * se_mean + 1e-14, (h, m1, mean_h)
        assert abs((m2 - m1 * m1) - var_h) <= 5.0 * se_var + 1e-14, (h, m2 - m1 * m1, var_h)
    assert abs(got["moments"][-1, 0, 0] - a ** hor * mean0) > 0.0      # (a sample, not the closed form copied)


def test_margin_condition():
    """a condition on the cases, not a measurement of the device: every threshold of every drawn pick of tests/test_particle_forecast.py
    keeps at least MARGIN S from every prefix sum"""
    smallest = np.inf
    for model, d, n, k, weights in DRAWN:
        lw = cloud_case(model, d, n, weights)[1]
        margin = pick_slots(np.zeros(n) if lw is None else lw, k, FC_SEED, 41)[1]
        smallest = min(smallest, margin)
        assert margin >= MARGIN, (model, d, n, k, weights, margin)
    for tag, start, n, k in BEHIND:
        ref = filter_reference(tag, start, n, 0.5)
        assert not ref["margins"] or min(ref["margins"]) >= MARGIN, (tag, start, n)
        margin = pick_slots(ref["lw"], k, SEED, int(case(tag)[0].n_pts))[1]
        smallest = min(smallest, margin)
        assert margin >= MARGIN, (tag, start, n, k, margin)
    for p in range(3):      # the batch of three of the GPU tests
        margin = pick_slots(cloud_case("L96", 12, 65, "random", p)[1], 17, FC_SEED, 41, index=p)[1]
        assert margin >= MARGIN, (p, margin)
        margin = pick_slots(cloud_case("L63", 3, 65, "random", p)[1], 17, FC_SEED, 41, index=p)[1]
        assert margin >= MARGIN, (p, margin)
    print("smallest margin of the picks:", smallest, "over", len(DRAWN) + len(BEHIND) + 6, "runs")


def test_the_pick_behind_the_filter_is_the_one_of_the_trajectories():
    """index0 = Np - 1: the uniform of the forecast's pick comes from counter (Np, 0, p, 0xffffffff), as that of vgpa_particle_paths"""
    lw = cloud_case("L96", 12, 65, "random")[1]
    q = shape_problem("L96", 12)
    got = forecast_numpy(q, cloud_case("L96", 12, 65, "random")[0], lw, 40, 0, 1, FC_SEED, 17)
    assert np.array_equal(got["slots"], pick_slots(lw, 17, FC_SEED, 41)[0])
    assert not np.array_equal(got["slots"], pick_slots(lw, 17, FC_SEED, 40)[0])


def test_record():
    q = shape_problem("L96", 5)
    cloud, lw = cloud_case("L96", 5, 17, "random")
    ref = forecast_numpy(q, cloud, lw, 40, 7, 3, FC_SEED, 4)
    rec = Forecast(lw, ref["moments"], ref["members"], ref["slots"], ref["state_end"], 40, 7, 3, 0.01, t0=1.0)
    assert len(rec) == 17 and rec.stride == 3 and rec.drawn
    assert np.array_equal(rec.grid, [40, 43, 46]) and np.allclose(rec.times, [1.4, 1.43, 1.46], rtol=1e-15)
    assert np.array_equal(rec.mean, ref["moments"][:, 0]) and rec.var.shape == (3, 5) and np.all(rec.var >= 0.0)
    assert np.array_equal(rec.var, np.maximum(ref["moments"][:, 1] - ref["moments"][:, 0] ** 2, 0.0))
    assert rec.members.shape == (4, 3, 5) and rec.state.shape == (17, 5) and np.array_equal(rec.log_w, lw) and rec.slots.shape == (4,)
    one = Forecast(np.zeros(3), np.zeros((1, 2, 1)), np.zeros((0, 1, 1)), [], np.ones((3, 1)), 0, 0, 1, 0.01, single_dim=True, drawn=False)
    assert one.mean.shape == (1,) and one.var.shape == (1,) and one.members.shape == (0, 1) and one.state.shape == (3,) and not one.drawn
    # a variance that rounding pushes below 0 is clipped
    flat = Forecast(np.zeros(2), np.array([[[1.0 + 1e-16], [1.0]]]), np.zeros((0, 1, 1)), [], np.ones((2, 1)), 5, 0, 1, 0.01)
    assert flat.var[0, 0] == 0.0
    for bad in (dict(horizon=-1), dict(stride=0), dict(index0=-1), dict(slots=[17, 0, 1, 2]), dict(moments=ref["moments"][:2])):
        args = dict(log_w=lw, moments=ref["moments"], members=ref["members"], slots=ref["slots"], state=ref["state_end"], index0=40, horizon=7,
                    stride=3, dt=0.01)
        args.update(bad)
        with pytest.raises(ValueError):
            Forecast(**args)


def test_symbol_and_prototype():
    assert "vgpa_particle_forecast" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header)
    assert _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_particle_forecast\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, const double* x_or_null, const double* x0_or_null, int32_t n_paths, uint64_t seed, double ess_fraction, "
                    "const double* prior_mu_or_null, const double* prior_tau_or_null, const double* cloud_or_null, "
                    "const double* cloud_logw_or_null, int32_t index0, int32_t horizon, int32_t stride, int32_t n_draw, "
                    "const int32_t* final_slots_or_null, double* logw, double* state, double* ess_or_null, int32_t* resampled_or_null, "
                    "double* moments, double* members_or_null, int32_t* slots_or_null, double* state_end_or_null")
    # the computation is stated in the header: the counter, the pick's counter, the two properties
    for phrase in ("(k0 + h, i, p, j)", "(k0 + 1, 0, p, 0xffffffff)", "bit for bit the last point of trajectory m of vgpa_particle_paths",
                   "states are equal bit for bit"):
        assert phrase in header, phrase


def test_python_surface():
    want = ["horizon", "n_paths", "seed", "stride", "n_draw", "ess_fraction", "x", "x0"]
    for owner, name, params in [(va.Context, "particle_forecast", want + ["cloud", "log_w", "index0", "slots"]),
                                (va.VarGP, "forecast", want + ["source", "cloud", "log_w", "index0", "slots"]),
                                (va.ProblemBatch, "forecast", want + ["source", "cloud", "log_w", "index0", "slots"])]:
        fn = getattr(owner, name, None)
        assert callable(fn), (owner.__name__, name)
        sig = inspect.signature(fn)
        got = list(sig.parameters)[1:]
        assert got[:len(params)] == params, (owner.__name__, name, got)
        assert sig.parameters["n_paths"].default is None and sig.parameters["seed"].default == 0 and sig.parameters["stride"].default == 1
        assert sig.parameters["n_draw"].default == 0 and sig.parameters["ess_fraction"].default == 0.5
    assert va.Forecast is Forecast and "Forecast" in va.__all__
    assert inspect.signature(va.VarGP.forecast).parameters["source"].default == "filter"
