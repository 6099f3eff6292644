"""
The call layout of the samplers and the particle entry points, without a device: what Context.sample_paths, sample_paths_weighted and the
ten particle_* methods hand to the C ABI, position by position, and what they refuse before they get there.

A Context is made with object.__new__ and given the attributes its methods read (B = 2, D = 3, Np = 11, n_obs = 2) and a `_lib` whose
entry points record their arguments and return 0.  Every call is made with pairwise distinct scalars, and is held against

  * the real entry's argtypes (va.load()): as many arguments, each of the kind its argtype takes;
  * the prototype of include/vgpa_hip.h, parsed: every scalar sits at the position of the parameter of its name, every input array is
    read back (at the time of the call) from the pointer at the position of its parameter, and every array of the result is the buffer
    whose address was passed at the position of its parameter, with the shape, dtype and fill value the method documents;
  * what was not asked for (history=False, per_particle=False, paths=False, no slots, no prior) is passed as null.

The recorder writes nothing, so the returned arrays still hold what the method filled them with.  The layout tests read the argtypes of the
built library (va.load()): they need libvgpa_hip.so, built as for every other test, and no device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from conftest import ROOT

B, D, NP, M = 2, 3, 11, 2
LEN_X = NP * D * (D + 1)
N, K, STRIDE, HORIZON, ESS_FRACTION, SEED, INDEX0 = 7, 5, 3, 9, 0.25, (1 << 40) + 12345, 13
N_KEEP, H_KEEP = (NP - 1) // STRIDE + 1, HORIZON // STRIDE + 1
RNG = np.random.default_rng(20)
X, X0 = RNG.standard_normal((B, LEN_X)), RNG.standard_normal((B, D))
PRIOR = (RNG.standard_normal((B, D)), RNG.standard_normal((B, D, D)))
LEVELS, SIDE = RNG.standard_normal((B, D)), np.array([1, -1, 1])
REF = RNG.standard_normal((NP, D))
SLOTS = np.array([[0, 6, 3, 3, 1], [2, 2, 5, 0, 4]])
CLOUD, CLOUD_LW = RNG.standard_normal((B, N, D)), RNG.standard_normal(N)
HANDLE = ctypes.c_void_p(0x5150)

with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as _fh:
    HEADER = _fh.read()

# the input arrays by the name of their parameter in the header: dtype and entries, for the recorder to read them while they are alive
INPUTS = {"x": (np.float64, B * LEN_X), "x0": (np.float64, B * D), "prior_mu": (np.float64, B * D), "prior_tau": (np.float64, B * D * D),
          "levels": (np.float64, B * D), "sides": (np.int32, B * D), "ref": (np.float64, B * NP * D), "final_slots": (np.int32, B * K),
          "cloud": (np.float64, B * N * D), "cloud_logw": (np.float64, B * N)}


def prototype(entry):
    """[(name without _or_null, kind)] of the entry's parameters in include/vgpa_hip.h; kind: "ptr", "f64", "u64", "i32" """
    found = re.search(r"int\s+" + entry + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert found, f"{entry}: prototype missing"
    out = []
    for decl in " ".join(found.group(1).split()).split(","):
        ctype, name = decl.strip().rsplit(" ", 1)
        kind = "ptr" if "*" in ctype else {"double": "f64", "uint64_t": "u64", "int32_t": "i32", "int": "i32"}[ctype]
        out.append((name[:-len("_or_null")] if name.endswith("_or_null") else name, kind))
    return out


class Recorder:
    """stands in for the ctypes handle: every entry point records (name, arguments, the input arrays behind them) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, entry):
        def call(*args):
            seen = {}
            if entry != "vgpa_destroy":
                for (name, _), arg in zip(prototype(entry), args):
                    if name in INPUTS and arg is not None:
                        dtype, count = INPUTS[name]
                        seen[name] = np.frombuffer(ctypes.string_at(arg.value, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
            self.calls.append((entry, args, seen))
            return 0
        return call


@pytest.fixture
def ctx():
    c = object.__new__(va.Context)
    c._lib, c._h = Recorder(), HANDLE
    c.B, c.D, c.Np, c.n_obs, c.len_x = B, D, NP, M, LEN_X
    yield c
    c._h = None


F64, I32 = np.float64, np.int32
FILTER_OUT = {"logw": ("log_w", (B, N), F64, None), "state": ("state", (B, N, D), F64, None), "ess": ("ess", (B, M), F64, 0),
              "resampled": ("resampled", (B, M), I32, 0)}
HISTORY = {"ancestors": ("ancestors", (B, M, N), I32, -1), "clouds": ("clouds", (B, M, N, D), F64, np.nan)}
WALK_IN = {"x": X, "x0": X0, "prior_mu": PRIOR[0], "prior_tau": PRIOR[1]}
COMMON = dict(x=X, x0=X0, prior=PRIOR)
FILTER_SCALARS = {"n_paths": N, "seed": SEED, "ess_fraction": ESS_FRACTION}


def case(method, entry, args, kwargs, scalars, ins, outs, nulls=(), result=None):
    return dict(method=method, entry=entry, args=args, kwargs=kwargs, scalars=scalars, ins=ins, outs=outs, nulls=nulls, result=result)


def smoothing_paths(method, slots):
    ins = dict(WALK_IN, final_slots=SLOTS) if slots else WALK_IN
    return case(method, "vgpa_" + method, (N, SEED, K), dict(COMMON, stride=STRIDE, ess_fraction=ESS_FRACTION, slots=SLOTS if slots else None),
                dict(FILTER_SCALARS, n_draw=K, stride=STRIDE), ins,
                dict(FILTER_OUT, paths=("paths", (B, K, N_KEEP, D), F64, None), slots=("slots", (B, M + 1, K), I32, -1)),
                () if slots else ("final_slots",))


FORECAST_OUT = {"moments": ("moments", (B, H_KEEP, 2, D), F64, None), "members": ("members", (B, K, H_KEEP, D), F64, None),
                "slots": ("slots", (B, K), I32, -1), "state_end": ("state_end", (B, N, D), F64, None)}
CASES = {
    "sample_paths": case("sample_paths", "vgpa_sample_paths", ("posterior", N, SEED), dict(stride=STRIDE, x=X, x0=X0),
                         {"kind": _lib.PATH_KINDS["posterior"], "n_paths": N, "stride": STRIDE, "seed": SEED}, {"x": X, "x0": X0},
                         {"out": (None, (B, N, N_KEEP, D), F64, None)}, result=lambda r: {None: r}),
    "sample_paths-model": case("sample_paths", "vgpa_sample_paths", ("model", N, SEED), dict(stride=STRIDE),
                               {"kind": _lib.PATH_KINDS["model"], "n_paths": N, "stride": STRIDE, "seed": SEED}, {},
                               {"out": (None, (B, N, N_KEEP, D), F64, None)}, ("x", "x0"), result=lambda r: {None: r}),
    "sample_paths_weighted": case("sample_paths_weighted", "vgpa_sample_paths_weighted", (N, SEED), dict(stride=STRIDE, x=X, x0=X0),
                                  {"n_paths": N, "stride": STRIDE, "seed": SEED}, {"x": X, "x0": X0},
                                  {"out": (0, (B, N, N_KEEP, D), F64, None), "logw": (1, (B, N, 2), F64, None), "start": (2, (B, N, D), F64, None)},
                                  result=lambda r: dict(enumerate(r))),
    "sample_paths_weighted-no-paths": case("sample_paths_weighted", "vgpa_sample_paths_weighted", (N, SEED), dict(stride=STRIDE, paths=False),
                                           {"n_paths": N, "stride": STRIDE, "seed": SEED}, {},
                                           {"logw": (1, (B, N, 2), F64, None), "start": (2, (B, N, D), F64, None)}, ("x", "x0", "out"),
                                           result=lambda r: dict(enumerate(r))),
    "particle_filter": case("particle_filter", "vgpa_particle_filter", (N, SEED), dict(COMMON, ess_fraction=ESS_FRACTION, history=True),
                            FILTER_SCALARS, WALK_IN, dict(FILTER_OUT, **HISTORY)),
    "particle_filter-bare": case("particle_filter", "vgpa_particle_filter", (N, SEED), dict(ess_fraction=ESS_FRACTION), FILTER_SCALARS, {},
                                 FILTER_OUT, ("x", "x0", "prior_mu", "prior_tau", "ancestors", "clouds")),
    "particle_statistics": case("particle_statistics", "vgpa_particle_statistics", (N, SEED), dict(COMMON, ess_fraction=ESS_FRACTION, per_particle=True),
                                FILTER_SCALARS, WALK_IN, dict(FILTER_OUT, stats=("stats", (B, N, 3, D), F64, None), mean=("mean", (B, 3, D), F64, None))),
    "particle_statistics-mean": case("particle_statistics", "vgpa_particle_statistics", (N, SEED), dict(COMMON, ess_fraction=ESS_FRACTION),
                                     FILTER_SCALARS, WALK_IN, dict(FILTER_OUT, mean=("mean", (B, 3, D), F64, None)), ("stats",)),
    "particle_events": case("particle_events", "vgpa_particle_events", (N, SEED, LEVELS), dict(COMMON, side=SIDE, stride=STRIDE, ess_fraction=ESS_FRACTION, per_particle=True),
                            dict(FILTER_SCALARS, stride=STRIDE), dict(WALK_IN, levels=LEVELS, sides=np.broadcast_to(SIDE, (B, D))),
                            dict(FILTER_OUT, rows=("rows", (B, N, 3, D), F64, None), mean=("mean", (B, 3, D), F64, None), cdf=("cdf", (B, N_KEEP, D), F64, None))),
    "particle_events-sums": case("particle_events", "vgpa_particle_events", (N, SEED, 0.5), dict(COMMON, side=-1, stride=STRIDE, ess_fraction=ESS_FRACTION),
                                 dict(FILTER_SCALARS, stride=STRIDE), dict(WALK_IN, levels=np.full((B, D), 0.5), sides=np.full((B, D), -1)),
                                 dict(FILTER_OUT, mean=("mean", (B, 3, D), F64, None), cdf=("cdf", (B, N_KEEP, D), F64, None)), ("rows",)),
    "particle_moments": case("particle_moments", "vgpa_particle_moments", (N, SEED), dict(COMMON, stride=STRIDE, ess_fraction=ESS_FRACTION),
                             dict(FILTER_SCALARS, stride=STRIDE), WALK_IN,
                             dict(FILTER_OUT, moments=("moments", (B, N_KEEP, 2, D), F64, None), lineage_ess=("lineage_ess", (B, M + 1), F64, 0))),
    "particle_covariance": case("particle_covariance", "vgpa_particle_covariance", (N, SEED), dict(COMMON, stride=STRIDE, ess_fraction=ESS_FRACTION),
                                dict(FILTER_SCALARS, stride=STRIDE), WALK_IN,
                                dict(FILTER_OUT, mean=("mean", (B, N_KEEP, D), F64, None), second=("second", (B, N_KEEP, D, D), F64, None),
                                     lineage_ess=("lineage_ess", (B, M + 1), F64, 0))),
    "particle_paths": smoothing_paths("particle_paths", False),
    "particle_paths-slots": smoothing_paths("particle_paths", True),
    "particle_backward_paths": smoothing_paths("particle_backward_paths", False),
    "particle_backward_paths-slots": smoothing_paths("particle_backward_paths", True),
    "particle_conditional": case("particle_conditional", "vgpa_particle_conditional", (REF, N, SEED), dict(COMMON, ess_fraction=ESS_FRACTION, history=True),
                                 FILTER_SCALARS, dict(WALK_IN, ref=np.broadcast_to(REF, (B, NP, D))),
                                 dict(FILTER_OUT, trajectory=("trajectory", (B, NP, D), F64, None), slots=("slots", (B, M + 1), I32, -1), **HISTORY)),
    "particle_conditional-bare": case("particle_conditional", "vgpa_particle_conditional", (np.broadcast_to(REF, (B, NP, D)), N, SEED),
                                      dict(COMMON, ess_fraction=ESS_FRACTION), FILTER_SCALARS, dict(WALK_IN, ref=np.broadcast_to(REF, (B, NP, D))),
                                      dict(FILTER_OUT, trajectory=("trajectory", (B, NP, D), F64, None), slots=("slots", (B, M + 1), I32, -1)),
                                      ("ancestors", "clouds")),
    "particle_forecast-filter": case("particle_forecast", "vgpa_particle_forecast", (HORIZON, N, SEED),
                                     dict(COMMON, stride=STRIDE, n_draw=K, ess_fraction=ESS_FRACTION),
                                     dict(FILTER_SCALARS, index0=0, horizon=HORIZON, stride=STRIDE, n_draw=K), WALK_IN, dict(FILTER_OUT, **FORECAST_OUT),
                                     ("cloud", "cloud_logw", "final_slots")),
    # a given cloud: no filter runs; the record's log_w and state are the caller's, the slots say how many members there are
    "particle_forecast-cloud": case("particle_forecast", "vgpa_particle_forecast", (HORIZON,),
                                    dict(seed=SEED, stride=STRIDE, ess_fraction=ESS_FRACTION, cloud=CLOUD, log_w=CLOUD_LW, index0=INDEX0, slots=SLOTS),
                                    dict(FILTER_SCALARS, index0=INDEX0, horizon=HORIZON, stride=STRIDE, n_draw=K),
                                    {"cloud": CLOUD, "cloud_logw": np.broadcast_to(CLOUD_LW, (B, N)), "final_slots": SLOTS}, FORECAST_OUT,
                                    ("x", "x0", "prior_mu", "prior_tau")),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_call_layout(ctx, tag):
    c = CASES[tag]
    res = getattr(ctx, c["method"])(*c["args"], **c["kwargs"])
    assert [entry for entry, _, _ in ctx._lib.calls] == [c["entry"]]      # one call of the library, of this entry
    _, args, seen = ctx._lib.calls[0]
    params, argtypes = prototype(c["entry"]), getattr(va.load(), c["entry"]).argtypes
    assert len(args) == len(argtypes) == len(params)
    assert args[0] is HANDLE
    at = {}
    for (name, kind), argtype, arg in zip(params, argtypes, args):      # every position holds what its argtype takes
        assert name not in at
        at[name] = arg
        if kind == "ptr":
            assert argtype is ctypes.c_void_p and (arg is None or isinstance(arg, ctypes.c_void_p)), name
            assert arg is None or arg.value, name
        elif kind == "f64":
            assert argtype is ctypes.c_double and type(arg) is float, name
        elif kind == "u64":
            assert argtype is ctypes.c_uint64 and type(arg) is int and 0 <= arg < 2 ** 64, name
        else:
            assert argtype in (ctypes.c_int32, ctypes.c_int) and type(arg) is int and -2 ** 31 <= arg < 2 ** 31, name
    scalars = {name for name, kind in params if kind != "ptr"}
    assert scalars == set(c["scalars"])                                  # every scalar of the prototype, at the position of its name
    for name, value in c["scalars"].items():
        assert at[name] == value, name
    assert set(seen) == set(c["ins"])                                    # the input arrays: these and no other, laid out for the whole batch
    for name, value in c["ins"].items():
        assert np.array_equal(seen[name], np.asarray(value).ravel()), name
    for name in c["nulls"]:
        assert at[name] is None, name
    got = res if c["result"] is None else c["result"](res)
    for name, (key, shape, dtype, fill) in c["outs"].items():           # the result's arrays are the buffers the library was given
        arr = got[key]
        assert at[name] is not None and at[name].value == arr.ctypes.data, name
        assert arr.shape == shape and arr.dtype == dtype and arr.flags["C_CONTIGUOUS"], name
        if fill is not None:
            assert np.all(np.isnan(arr)) if np.isnan(fill) else np.all(arr == fill), name
    if "out" in c["nulls"]:                                               # ... and what was not asked for is None in the result too
        assert got[0] is None
    pointers = {name for name, kind in params if kind == "ptr"} - {"ctx"}
    if tag != "particle_forecast-cloud":
        assert pointers == set(c["ins"]) | set(c["outs"]) | set(c["nulls"])  # nothing of the prototype went unlooked at
    if isinstance(res, dict):
        keys = [key for key, _, _, _ in c["outs"].values()]
        extra = {"particle_forecast": ["index0"]}.get(c["method"], [])
        nulled = [n for n in c["nulls"] if n in ("ancestors", "clouds", "stats", "rows")]
        assert sorted(res) == sorted(keys + extra + nulled + (["log_w", "state", "ess", "resampled"] if tag == "particle_forecast-cloud" else []))
        assert list(res)[:4] == ["log_w", "state", "ess", "resampled"]
        for name in nulled:
            assert res[name] is None


def test_forecast_record_of_a_given_cloud(ctx):
    """the dict behind a given cloud: log_w and state are the caller's (equal weights: zeros), no ess, no resampled, index0 as given or Np - 1"""
    c = CASES["particle_forecast-cloud"]
    res = ctx.particle_forecast(*c["args"], **c["kwargs"])
    assert np.array_equal(res["log_w"], np.broadcast_to(CLOUD_LW, (B, N))) and np.array_equal(res["state"], CLOUD)
    assert res["ess"] is None and res["resampled"] is None and res["index0"] == INDEX0
    args = ctx._lib.calls[0][1]
    names = [name for name, _ in prototype("vgpa_particle_forecast")]
    for name in ("logw", "state", "ess", "resampled"):                  # (the library is still given the four buffers)
        assert args[names.index(name)] is not None
    res = ctx.particle_forecast(HORIZON, cloud=CLOUD[0])
    assert np.array_equal(res["log_w"], np.zeros((B, N))) and np.array_equal(res["state"], np.broadcast_to(CLOUD[0], (B, N, D)))
    assert res["index0"] == NP - 1 and res["members"].shape == (B, 0, HORIZON + 1, D) and res["slots"].shape == (B, 0)
    args = ctx._lib.calls[1][1]
    assert args[names.index("index0")] == NP - 1 and args[names.index("n_draw")] == 0 and args[names.index("cloud_logw")] is None
    assert args[names.index("stride")] == 1 and args[names.index("seed")] == 0 and args[names.index("n_paths")] == N
    res = ctx.particle_forecast(HORIZON, N, SEED)                       # behind the filter index0 is passed as 0 and reported as Np - 1
    assert res["index0"] == NP - 1 and ctx._lib.calls[2][1][names.index("index0")] == 0


def test_seed_is_taken_modulo_2_64(ctx):
    ctx.particle_filter(N, -1)
    ctx.sample_paths("posterior", N, 2 ** 64 + 5)
    assert ctx._lib.calls[0][1][4] == 2 ** 64 - 1 and ctx._lib.calls[1][1][6] == 5


BIG = 2 ** 31
X_BAD, X_TEXT = np.zeros(5), f"x has 5 entries, expected {B * LEN_X}"
REFUSALS = [
    # the integers of the C ABI, named in the order of the call
    (lambda c: c.sample_paths("posterior", BIG, 1, stride=STRIDE, x=X_BAD), f"n_paths and stride must fit into 32 bits (n_paths = {BIG}, stride = 3)"),
    (lambda c: c.sample_paths_weighted(N, 1, stride=-BIG - 1, x=X_BAD), f"n_paths and stride must fit into 32 bits (n_paths = 7, stride = {-BIG - 1})"),
    (lambda c: c.particle_filter(BIG, 1, x=X_BAD), f"n_paths must fit into 32 bits (n_paths = {BIG})"),
    (lambda c: c.particle_statistics(BIG, 1, x=X_BAD), f"n_paths must fit into 32 bits (n_paths = {BIG})"),
    (lambda c: c.particle_events(N, 1, [0.0] * 4, stride=BIG), f"n_paths and stride must fit into 32 bits (n_paths = 7, stride = {BIG})"),
    (lambda c: c.particle_moments(N, 1, stride=BIG, x=X_BAD), f"n_paths and stride must fit into 32 bits (n_paths = 7, stride = {BIG})"),
    (lambda c: c.particle_covariance(BIG, 1, x=X_BAD), f"n_paths and stride must fit into 32 bits (n_paths = {BIG}, stride = 1)"),
    (lambda c: c.particle_paths(N, 1, BIG, x=X_BAD), f"n_paths, n_draw and stride must fit into 32 bits (n_paths = 7, n_draw = {BIG}, stride = 1)"),
    (lambda c: c.particle_backward_paths(BIG, 1, K, stride=STRIDE, x=X_BAD),
     f"n_paths, n_draw and stride must fit into 32 bits (n_paths = {BIG}, n_draw = 5, stride = 3)"),
    (lambda c: c.particle_conditional(np.zeros(4), BIG, 1, x=X_BAD), f"n_paths must fit into 32 bits (n_paths = {BIG})"),
    (lambda c: c.particle_forecast(BIG, N, 1, x=X_BAD),
     f"n_paths, n_draw, stride, horizon and index0 must fit into 32 bits (n_paths = 7, n_draw = 0, stride = 1, horizon = {BIG}, index0 = 10)"),
    (lambda c: c.particle_forecast(HORIZON, cloud=CLOUD, index0=BIG, x=X_BAD),
     f"n_paths, n_draw, stride, horizon and index0 must fit into 32 bits (n_paths = 7, n_draw = 0, stride = 1, horizon = 9, index0 = {BIG})"),
    (lambda c: c.lag_covariance([0], stride=BIG, x=X_BAD), f"n_anchor and stride must fit into 32 bits (n_anchor = 1, stride = {BIG})"),
    # x, behind them
    (lambda c: c.sample_paths("posterior", N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.sample_paths_weighted(N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.particle_filter(N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.particle_statistics(N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.particle_events(N, 1, 0.0, x=X_BAD), X_TEXT),
    (lambda c: c.particle_moments(N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.particle_covariance(N, 1, x=X_BAD), X_TEXT),
    (lambda c: c.particle_paths(N, 1, K, x=X_BAD, slots=[0.5]), X_TEXT),            # (before the slots)
    (lambda c: c.particle_backward_paths(N, 1, K, x=X_BAD, slots=[0.5]), X_TEXT),
    (lambda c: c.particle_conditional(np.zeros(4), N, 1, x=X_BAD), X_TEXT),         # (before ref)
    (lambda c: c.particle_forecast(HORIZON, N, 1, x=X_BAD, slots=[0.5]), X_TEXT),
    (lambda c: c.lag_covariance([0], kind="propagator", x=X_BAD), X_TEXT),
    (lambda c: c.lag_covariance([0], x=X_BAD), X_TEXT),
    # unknown kinds come first
    (lambda c: c.sample_paths("prior", BIG, 1), " Unknown kind of paths -> prior"),
    (lambda c: c.lag_covariance([0.5], kind="lag"), " Unknown kind of lag covariance -> lag"),
    (lambda c: c.lag_covariance([0.5], stride=BIG), "anchors must be a 1-D sequence of integer grid indices"),
    # levels and sides: behind the integers, before x
    (lambda c: c.particle_events(N, 1, [0.0] * 4, side=2, x=X_BAD), f"levels has 4 entries, expected 1, {D} or {B * D}"),
    (lambda c: c.particle_events(N, 1, [0.0, np.inf, 0.0], side=2, x=X_BAD), "levels must be finite"),
    (lambda c: c.particle_events(N, 1, 0.0, side=[1, 1], x=X_BAD), f"side has 2 entries, expected 1, {D} or {B * D}"),
    (lambda c: c.particle_events(N, 1, 0.0, side=[1, 0, -1], x=X_BAD), "side must be +1 or -1"),
    # slots
    (lambda c: c.particle_paths(N, 1, K, slots=[0.5] * K), "slots must be integers that fit into 32 bits"),
    (lambda c: c.particle_backward_paths(N, 1, K, slots=[BIG] * K), "slots must be integers that fit into 32 bits"),
    (lambda c: c.particle_paths(N, 1, K, slots=np.zeros((0,), dtype=int)), "slots must be integers that fit into 32 bits"),
    (lambda c: c.particle_forecast(HORIZON, N, 1, slots=[-BIG - 1]), "slots must be integers that fit into 32 bits"),
    # ref
    (lambda c: c.particle_conditional(np.zeros(4), N, 1), f"ref has 4 entries, expected {B} x {NP} x {D}"),
    # the forecast's cloud, before everything else of the call
    (lambda c: c.particle_forecast(BIG, cloud=np.zeros((N, D + 1))), f"cloud must be (B, n, {D}) or (n, {D})"),
    (lambda c: c.particle_forecast(BIG, cloud=np.zeros(D)), f"cloud must be (B, n, {D}) or (n, {D})"),
    (lambda c: c.particle_forecast(BIG, cloud=np.zeros((0, D))), f"cloud must be (B, n, {D}) or (n, {D})"),
    (lambda c: c.particle_forecast(BIG, N + 1, cloud=CLOUD), f"n_paths = {N + 1}, but the cloud has {N} particles"),
    (lambda c: c.particle_forecast(BIG), "n_paths is needed where no cloud is given"),
    (lambda c: c.particle_forecast(BIG, N, log_w=CLOUD_LW), "log_w and index0 belong to a given cloud"),
    (lambda c: c.particle_forecast(BIG, N, index0=3), "log_w and index0 belong to a given cloud"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_by_text_and_order(ctx, i):
    """each call is wrong in more than one way where the order matters: the text says which check fired first.  Nothing reaches the library."""
    call, text = REFUSALS[i]
    with pytest.raises(ValueError) as err:
        call(ctx)
    assert str(err.value) == text
    assert ctx._lib.calls == []


def _records():
    """what the six records of the filter's walk refuse, by text: each case is wrong in the way named first and, where the order of the
    checks matters, in a later way too"""
    z1, ok = np.zeros((3, 1)), dict(ess=[1.0], resampled=[0])
    odd = dict(ess=[1.0], resampled=[])
    mom, mean, second, paths = np.zeros((4, 2, 1)), np.zeros((4, 1)), np.zeros((4, 1, 1)), np.zeros((2, 4, 1))
    return [
        (lambda: va.ParticleFilterResult([], z1, [1.0], []), " ParticleFilterResult: at least one particle."),
        (lambda: va.ParticleFilterResult([0.0, 0.0], z1, [1.0], [0], np.zeros((3, 3))), " ParticleFilterResult: log_w, state, ess and resampled do not belong together."),
        (lambda: va.ParticleFilterResult([0.0] * 3, z1, [1.0], [], np.zeros((3, 3))), " ParticleFilterResult: log_w, state, ess and resampled do not belong together."),
        (lambda: va.ParticleFilterResult([0.0] * 3, z1, [1.0], [0], np.zeros((3, 3))), " ParticleFilterResult: ancestors must be (observations, particles)."),
        (lambda: va.PathStatistics([], np.zeros((2, 1)), 0.01, 10, "XX"), " PathStatistics: at least one particle."),
        (lambda: va.PathStatistics([0.0], np.zeros((2, 1)), 0.01, 10, "XX", **odd), " PathStatistics: mean must be (3, D)."),
        (lambda: va.PathStatistics([0.0], z1, 0.01, 10, "XX", **odd), " PathStatistics: unknown model -> XX"),
        (lambda: va.PathStatistics([0.0], z1, 0.01, 10, "OU", rows=z1, **odd), " PathStatistics: rows must be (particles, 3, D)."),
        (lambda: va.PathStatistics([0.0], z1, 0.01, 10, "OU", rows=z1[None], **odd), " PathStatistics: ess and resampled do not belong together."),
        (lambda: va.PathEvents([], z1, mean, 0.0, 1, 0, 11, 0.01), " PathEvents: at least one particle."),
        (lambda: va.PathEvents([0.0], z1[:2], mean, 0.0, 1, 0, 11, 0.01), " PathEvents: mean must be (3, D)."),
        (lambda: va.PathEvents([0.0], z1, mean[:3], 0.0, 1, 0, 11, 0.01), " PathEvents: stride and n_pts must be at least 1."),
        (lambda: va.PathEvents([0.0], z1, mean[:3], 0.0, 1, 3, 0, 0.01), " PathEvents: stride and n_pts must be at least 1."),
        (lambda: va.PathEvents([0.0], z1, mean[:3], 0.0, 2, 3, 11, 0.01), " PathEvents: cdf must be (n_keep, D)."),
        (lambda: va.PathEvents([0.0], z1, mean, 0.0, 2, 3, 11, 0.01, rows=z1), " PathEvents: side must be +1 or -1."),
        (lambda: va.PathEvents([0.0], z1, mean, 0.0, -1, 3, 11, 0.01, rows=z1, **odd), " PathEvents: rows must be (particles, 3, D)."),
        (lambda: va.PathEvents([0.0], z1, mean, 0.0, -1, 3, 11, 0.01, **odd), " PathEvents: ess and resampled do not belong together."),
        (lambda: va.SmoothingMoments([], mom, 0, 11, [5], [1.0]), " SmoothingMoments: at least one particle."),
        (lambda: va.SmoothingMoments([0.0], mom[:3], 0, 11, [5], [1.0]), " SmoothingMoments: stride and n_pts must be at least 1."),
        (lambda: va.SmoothingMoments([0.0], mom[:3], 3, 11, [5], [1.0]), " SmoothingMoments: moments must be (n_keep, 2, D)."),
        (lambda: va.SmoothingMoments([0.0], mom, 3, 11, [5], [1.0], **ok), " SmoothingMoments: obs_t, lineage_ess, ess and resampled do not belong together."),
        (lambda: va.SmoothingMoments([0.0], mom, 3, 11, [5], [1.0, 1.0], **odd), " SmoothingMoments: obs_t, lineage_ess, ess and resampled do not belong together."),
        (lambda: va.SmoothingCovariance([], mean, second, 0, 11, [5], [1.0]), " SmoothingCovariance: at least one particle."),
        (lambda: va.SmoothingCovariance([0.0], mean[:3], second, 3, 0, [5], [1.0]), " SmoothingCovariance: stride and n_pts must be at least 1."),
        (lambda: va.SmoothingCovariance([0.0], mean[:3], second, 3, 11, [5], [1.0]), " SmoothingCovariance: mean must be (n_keep, D) and second (n_keep, D, D)."),
        (lambda: va.SmoothingCovariance([0.0], mean, second, 3, 11, [5], [1.0], **ok), " SmoothingCovariance: obs_t, lineage_ess, ess and resampled do not belong together."),
        (lambda: va.SmoothingCovariance([0.0], mean, second, 3, 11, [5], [1.0, 1.0], **odd), " SmoothingCovariance: obs_t, lineage_ess, ess and resampled do not belong together."),
        (lambda: va.SmoothingPaths([], paths, [[0, 0]], 0, 11, []), " SmoothingPaths: at least one particle."),
        (lambda: va.SmoothingPaths([0.0], paths[:, :3], [[0, 0]], 0, 11, []), " SmoothingPaths: stride and n_pts must be at least 1."),
        (lambda: va.SmoothingPaths([0.0], paths[:, :3], [[0, 0]], 3, 11, []), " SmoothingPaths: paths must be (K, n_keep, D)."),
        (lambda: va.SmoothingPaths([0.0], paths, [[0, 0]], 3, 11, [5]), " SmoothingPaths: slots must be (M + 1, K)."),
        (lambda: va.SmoothingPaths([0.0], paths, [[0, 1]], 3, 11, [], **odd), " SmoothingPaths: a slot outside [0, n)."),
        (lambda: va.SmoothingPaths([0.0], paths, [[0, 0]], 3, 11, [], method="other", **odd), " SmoothingPaths: ess and resampled do not belong together."),
        (lambda: va.SmoothingPaths([0.0], paths, [[0, 0]], 3, 11, [], method="other"), " SmoothingPaths: method is 'genealogy' or 'backward'."),
    ]


@pytest.mark.parametrize("i", range(len(_records())))
def test_records_refuse_by_text_and_in_order(i):
    make, text = _records()[i]
    with pytest.raises(ValueError) as err:
        make()
    assert str(err.value) == text


def test_records_share_what_they_have():
    """what the records of the walk answer alike: log_evidence, the normalised weights, len, grid and the stretch of a kept index"""
    lw = np.array([-1.0, 0.5, -3.0])
    want = float(np.log(np.mean(np.exp(lw))))
    w = np.exp(lw - lw.max()) / np.sum(np.exp(lw - lw.max()))
    flt = va.ParticleFilterResult(lw, np.zeros((3, 1)), [2.0], [1])
    sta = va.PathStatistics(lw, np.zeros((3, 1)), 0.01, 10, "OU")
    evt = va.PathEvents(lw, np.zeros((3, 1)), np.zeros((4, 1)), 0.0, 1, 3, 11, 0.01)
    mom = va.SmoothingMoments(lw, np.zeros((4, 2, 1)), 3, 11, [3, 7], [1.0, 2.0, 3.0])
    cov = va.SmoothingCovariance(lw, np.zeros((4, 1)), np.zeros((4, 1, 1)), 3, 11, [3, 7], [1.0, 2.0, 3.0])
    pth = va.SmoothingPaths(lw, np.zeros((2, 4, 1)), [[0, 0], [0, 1], [2, 1]], 3, 11, [3, 7])
    for rec in (flt, sta, evt, mom, cov, pth):
        assert abs(rec.log_evidence() - want) < 1e-14 and type(rec.log_evidence()) is float and rec.log_evidence() == flt.log_evidence()
        assert len(rec) == (2 if rec is pth else 3)
    assert np.array_equal(flt._normalised(), w) and np.array_equal(evt.weights(), w) and np.array_equal(flt.mean(np.eye(3)), w)
    assert abs(flt.final_ess() - 1.0 / np.sum(w * w)) < 1e-12
    for rec in (evt, mom, cov, pth):
        assert np.array_equal(rec.grid, [0, 3, 6, 9]) and rec.grid.dtype == np.int64 and (rec.stride, rec.n_pts) == (3, 11)
    assert np.array_equal(mom.lineage_ess_on_grid(), [1.0, 1.0, 2.0, 3.0]) and np.array_equal(cov.lineage_ess_on_grid(), [1.0, 1.0, 2.0, 3.0])
    assert np.array_equal(pth.distinct(), [1, 2, 2]) and np.array_equal(pth.distinct_on_grid(), [1, 1, 2, 2])
    assert "grid" in vars(evt)                                          # (PathEvents holds its grid; the others compute it)


def test_event_inputs_on_a_bare_namespace():
    """Context._event_inputs reads B and D alone (tests/test_particle_events_cpu.py lays levels and sides out with it)"""
    import types
    lev, sd = va.Context._event_inputs(types.SimpleNamespace(B=B, D=D), 0.25, SIDE)
    assert lev.shape == sd.shape == (B, D) and lev.dtype == F64 and sd.dtype == I32 and lev.flags["C_CONTIGUOUS"] and sd.flags["C_CONTIGUOUS"]
    assert np.all(lev == 0.25) and np.array_equal(sd, np.broadcast_to(SIDE, (B, D)))
