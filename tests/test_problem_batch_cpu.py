"""ProblemBatch refuses members that cannot share one context, before any device work (no GPU needed)."""
import pytest

import vgpa_amd as va
from helpers import SEED, build_problem


def test_problem_batch_names_the_first_field_that_differs():
    a = build_problem("OU", "euler", 2.0, seed=SEED)
    b = build_problem("OU", "euler", 2.0, seed=SEED + 1)
    va.ProblemBatch([a["vgp"], b["vgp"]])                        # own data, same configuration: accepted
    c = build_problem("OU", "heun", 2.0, seed=SEED + 2)
    with pytest.raises(ValueError, match="'method'"):
        va.ProblemBatch([a["vgp"], c["vgp"]])
    d = build_problem("OU", "euler", 3.0, seed=SEED + 3)
    with pytest.raises(ValueError, match="'Np'"):
        va.ProblemBatch([a["vgp"], d["vgp"]])
    e = build_problem("DW", "euler", 2.0, seed=SEED)
    with pytest.raises(ValueError, match="'model'"):
        va.ProblemBatch([a["vgp"], e["vgp"]])
    f = build_problem("OU", "euler", 2.0, seed=SEED + 4)
    f["model"].theta = 0.5
    with pytest.raises(ValueError, match="'theta'"):
        va.ProblemBatch([a["vgp"], f["vgp"]])


def test_context_exports_set_problem_data():
    assert "vgpa_set_problem_data" in va._lib.SYMBOLS
    assert hasattr(va.Context, "set_problem_data")
