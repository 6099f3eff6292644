"""Per-problem observation count, noise and operator (vgpa_set_problem_obs_model / ProblemBatch(own_observations=True)): the
interface and the host-side stacking of padded rows, without a device."""
import inspect
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd.batch import stack_observations
from helpers import SEED, build_problem

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vgpa_hip.h")
PROTOTYPE = ("int vgpa_set_problem_obs_model(vgpa_ctx* ctx, const int32_t* n_obs, const double* obs_noise, "
             "const double* obs_h);")


def _rewired(p, obs_t, obs_y, obs_noise, obs_h=None):
    """p's VarGP with another likelihood: its own observation count, noise R and operator H"""
    single = p["model"].single_dim
    lik = va.GaussianLikelihood(obs_y, obs_t, obs_noise, obs_h, single)
    return va.VarGP(p["model"], p["m0"], p["s0"], p["fwd"], p["bwd"], lik, p["kl0"], obs_y, obs_t)


def test_symbol_prototype_and_abi_version():
    assert "vgpa_set_problem_obs_model" in va._lib.SYMBOLS
    with open(HEADER) as fh:
        text = fh.read()
    assert PROTOTYPE in re.sub(r"\s+", " ", text)
    assert va._lib.ABI_VERSION == 2
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", text)


def test_context_and_batch_have_the_new_method_and_keyword():
    assert hasattr(va.Context, "set_problem_obs_model")
    assert list(inspect.signature(va.Context.set_problem_obs_model).parameters)[1:] == ["n_obs", "obs_noise", "obs_h"]
    sig = inspect.signature(va.ProblemBatch.__init__)
    assert sig.parameters["own_observations"].default is False


def test_stack_observations_pads_beyond_each_count():
    rng = np.random.default_rng(5)
    d, counts = 3, (4, 2, 1, 4)
    rows = []
    for k, m in enumerate(counts):
        rows.append(dict(obs_t=np.arange(1, m + 1) * (k + 2), obs_y=rng.standard_normal((m, d)),
                         obs_noise=(1.0 + k) * np.eye(d), obs_h=None if k % 2 == 0 else np.diag([1.0, 0.0, 1.0])))
    out = stack_observations(rows)
    assert out["n_obs"].dtype == np.int32 and out["n_obs"].tolist() == list(counts)
    assert out["obs_t"].shape == (4, 4) and out["obs_t"].dtype == np.int64
    assert out["obs_y"].shape == (4, 4, d) and out["obs_noise"].shape == (4, d, d) and out["obs_h"].shape == (4, d, d)
    for k, m in enumerate(counts):
        assert np.array_equal(out["obs_t"][k, :m], rows[k]["obs_t"]) and np.all(out["obs_t"][k, m:] == -1)
        assert np.array_equal(out["obs_y"][k, :m], rows[k]["obs_y"]) and np.all(np.isnan(out["obs_y"][k, m:]))
        assert not np.any(np.isnan(out["obs_y"][k, :m]))
        assert np.array_equal(out["obs_noise"][k], rows[k]["obs_noise"])
        # a member without an operator among members with one: the identity
        assert np.array_equal(out["obs_h"][k], np.eye(d) if rows[k]["obs_h"] is None else rows[k]["obs_h"])
    for r in rows:
        r["obs_h"] = None
    assert stack_observations(rows)["obs_h"] is None
    one_d = [dict(obs_t=np.array([3, 9]), obs_y=np.array([0.5, -0.5]), obs_noise=np.array([[0.04]]), obs_h=None),
             dict(obs_t=np.array([4]), obs_y=np.array([0.25]), obs_noise=np.array([[0.08]]), obs_h=None)]
    out = stack_observations(one_d)
    assert out["obs_y"].shape == (2, 2, 1) and out["obs_noise"].shape == (2, 1, 1) and np.isnan(out["obs_y"][1, 1, 0])
    with pytest.raises(ValueError, match="at least one observation"):
        stack_observations([one_d[0], dict(obs_t=np.array([], dtype=int), obs_y=np.array([]), obs_noise=np.array([[1.0]]), obs_h=None)])


def test_own_observations_accepts_members_that_differ_in_m_r_and_h():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    b = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    c = build_problem("OU", "euler", 2.0, seed=SEED + 2)
    m = len(a["obs_t"])
    vb = _rewired(b, b["obs_t"][:-1], b["obs_y"][:-1], 2.0 * b["obs_noise"])
    vc = _rewired(c, c["obs_t"][:1], c["obs_y"][:1], c["obs_noise"])
    pb = va.ProblemBatch([a["vgp"], vb, vc], own_observations=True)
    assert pb.B == 3 and pb.own_observations and not pb.own_parameters
    pp, _ = pb._per_problem()
    assert pp["n_obs"].tolist() == [m, m - 1, 1]
    assert pp["obs_t"].shape == (3, m) and pp["obs_y"].shape == (3, m, 1) and pp["obs_noise"].shape == (3, 1, 1)
    assert np.all(pp["obs_t"][1, m - 1:] == -1) and np.all(pp["obs_t"][2, 1:] == -1)
    assert np.all(np.isnan(pp["obs_y"][1, m - 1:])) and np.all(np.isnan(pp["obs_y"][2, 1:]))
    assert np.array_equal(pp["obs_t"][1, :m - 1], np.asarray(b["obs_t"][:-1]))
    assert pp["obs_noise"][1, 0, 0] == 2.0 * pp["obs_noise"][0, 0, 0]
    assert "obs_h" not in pp and pb._ctx is None        # (no context was created)
    # n-D members: their own operator and dense noise, combined with own parameters
    e = build_problem("L63", "rk4", 1.0, seed=SEED)
    f = build_problem("L63", "rk4", 1.0, seed=SEED + 1)
    f["model"].theta = [9.0, 27.0, 2.5]
    h = np.diag([1.0, 0.0, 1.0])
    r = np.asarray(f["obs_noise"]) * (0.8 * np.eye(3) + 0.2)
    vf = _rewired(f, f["obs_t"][:-2], f["obs_y"][:-2], r, h)
    pb = va.ProblemBatch([e["vgp"], vf], own_parameters=True, own_observations=True)
    pp, _ = pb._per_problem()
    assert pp["n_obs"].tolist() == [len(e["obs_t"]), len(e["obs_t"]) - 2]
    assert np.array_equal(pp["obs_h"][0], np.eye(3)) and np.array_equal(pp["obs_h"][1], h) and np.array_equal(pp["obs_noise"][1], r)
    assert pp["theta"].shape == (2, 3)


def test_own_observations_still_names_the_other_shared_fields():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    with pytest.raises(ValueError, match="'method'"):
        va.ProblemBatch([a["vgp"], build_problem("OU", "heun", 2.0, seed=SEED + 1)["vgp"]], own_observations=True)
    b = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    b["model"].theta = 0.5
    with pytest.raises(ValueError, match="'theta'"):
        va.ProblemBatch([a["vgp"], b["vgp"]], own_observations=True)


def test_default_batch_keeps_its_errors_word_for_word():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    r = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    shares = "a batch shares the model class, theta, sigma, dt, Np, method, R, H and the observation count M."
    with pytest.raises(ValueError) as err:
        va.ProblemBatch([a["vgp"], _rewired(r, r["obs_t"], r["obs_y"], 2.0 * r["obs_noise"])])
    assert str(err.value) == " ProblemBatch: problem 1 differs from problem 0 in 'R'; " + shares
    with pytest.raises(ValueError) as err:
        va.ProblemBatch([a["vgp"], _rewired(r, r["obs_t"][:-1], r["obs_y"][:-1], r["obs_noise"])])
    assert str(err.value) == " ProblemBatch: problem 1 differs from problem 0 in 'M'; " + shares
    e = build_problem("L63", "rk4", 1.0, seed=SEED)
    f = build_problem("L63", "rk4", 1.0, seed=SEED + 1)
    with pytest.raises(ValueError) as err:
        va.ProblemBatch([e["vgp"], _rewired(f, f["obs_t"], f["obs_y"], f["obs_noise"], np.diag([1.0, 0.0, 1.0]))])
    assert str(err.value) == " ProblemBatch: problem 1 differs from problem 0 in 'H'; " + shares
