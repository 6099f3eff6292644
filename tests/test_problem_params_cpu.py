"""Per-problem parameters (vgpa_set_problem_params / ProblemBatch(own_parameters=True)): the interface, without a device."""
import pytest

import vgpa_amd as va
from helpers import SEED, build_problem


def test_set_problem_params_is_exported():
    assert "vgpa_set_problem_params" in va._lib.SYMBOLS


def test_context_has_set_problem_params():
    assert hasattr(va.Context, "set_problem_params")


def test_own_parameters_accepts_members_that_differ_in_theta_and_sigma():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    b = build_problem("OU", "euler", 2.0, seed=SEED)
    b["model"].theta = 0.5
    c = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    c["model"].sigma = 0.7
    d = build_problem("OU", "euler", 2.0, seed=SEED + 2)
    d["model"].theta, d["model"].sigma = 1.5, 0.3
    pb = va.ProblemBatch([a["vgp"], b["vgp"], c["vgp"], d["vgp"]], own_parameters=True)
    assert pb.B == 4 and pb.own_parameters
    e = build_problem("L63", "rk4", 1.0, seed=SEED)
    f = build_problem("L63", "rk4", 1.0, seed=SEED)
    f["model"].theta = [9.0, 27.0, 2.5]
    va.ProblemBatch([e["vgp"], f["vgp"]], own_parameters=True)


def test_own_parameters_still_names_the_other_shared_fields():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    with pytest.raises(ValueError, match="'method'"):
        va.ProblemBatch([a["vgp"], build_problem("OU", "heun", 2.0, seed=SEED + 1)["vgp"]], own_parameters=True)
    with pytest.raises(ValueError, match="'Np'"):
        va.ProblemBatch([a["vgp"], build_problem("OU", "euler", 3.0, seed=SEED + 1)["vgp"]], own_parameters=True)
    with pytest.raises(ValueError, match="'model'"):
        va.ProblemBatch([a["vgp"], build_problem("DW", "euler", 2.0, seed=SEED)["vgp"]], own_parameters=True)
    r = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    with pytest.raises(ValueError, match="'R'"):
        va.ProblemBatch([a["vgp"], _rewired(r, r["obs_t"], r["obs_y"], 2.0 * r["obs_noise"])], own_parameters=True)
    with pytest.raises(ValueError, match="'M'"):
        va.ProblemBatch([a["vgp"], _rewired(r, r["obs_t"][:-1], r["obs_y"][:-1], r["obs_noise"])], own_parameters=True)


def _rewired(p, obs_t, obs_y, obs_noise):
    """p's VarGP with another likelihood (observation noise R / observation count M)"""
    lik = va.GaussianLikelihood(obs_y, obs_t, obs_noise, None, True)
    return va.VarGP(p["model"], p["m0"], p["s0"], p["fwd"], p["bwd"], lik, p["kl0"], obs_y, obs_t)


def test_default_batch_still_refuses_theta_and_sigma():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    b = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    b["model"].theta = 0.5
    with pytest.raises(ValueError, match="'theta'"):
        va.ProblemBatch([a["vgp"], b["vgp"]])
    c = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    c["model"].sigma = 0.7
    with pytest.raises(ValueError, match="'sigma'"):
        va.ProblemBatch([a["vgp"], c["vgp"]])
