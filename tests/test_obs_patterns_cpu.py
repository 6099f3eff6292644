"""
CPU side of the observation-placement tests (tests/obs_patterns.py): the patterns themselves, the oracle's two modes on every one of
them, the ownership rule the GPU tests take their rank seams from, and the reference-generated fixtures of the `every` / `late`
placements.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, rel_err
from obs_patterns import NAMES, chunk_seams, time_chunk_seams, expected_count, lane_seams, pad_rows, patterns, rank_seams, time_slice
from oracle import vgpa_oracle as vo

GRIDS = (2, 3, 5, 8, 10, 11, 13, 34, 260)
SEAMS_13 = (4, 8, 12)


@pytest.mark.parametrize("n_pts", GRIDS)
def test_pattern_properties(n_pts):
    seams = (0, n_pts // 2, n_pts - 1)
    pats = patterns(n_pts, seams)
    assert set(pats) <= set(NAMES) and list(patterns(n_pts)) == [k for k in pats if k != "seams"]
    for name, idx in pats.items():
        assert idx.dtype == np.int64 and idx.ndim == 1 and idx.size >= 1, name
        assert np.all(np.diff(idx) > 0), name                              # strictly increasing
        assert idx[0] >= 0 and idx[-1] < n_pts, name
        if name != "seams":
            assert idx.size == expected_count(name, n_pts), name
    for name in NAMES[:-1]:
        assert (name in pats) == (expected_count(name, n_pts) is not None), name
    assert np.array_equal(pats["every"], np.arange(n_pts))
    assert pats["ends"].tolist() == [0, n_pts - 1]
    assert pats["late"][-1] == n_pts - 1 and pats["late"].size == -(-n_pts // 2)
    want = sorted({t for s in seams for t in (s - 1, s, s + 1) if 0 <= t < n_pts})
    assert pats["seams"].tolist() == want
    if n_pts >= 8:
        assert len(pats) == 8
        assert pats["inner"].tolist() == list(range(1, n_pts - 1))
        assert pats["head"].tolist() == [0, 1, 2] and pats["tail"].tolist() == [n_pts - 3, n_pts - 2, n_pts - 1]
        run = pats["run"].tolist()
        assert run[:3] == [2, 3, 4] and run[3] - run[2] > 1 and run[3] < n_pts - 1
        # what the equidistant sets never have: neighbours, the last grid point, a counter n far behind its grid index
        assert np.any(np.diff(pats["run"]) == 1) and pats["late"][0] - 0 >= n_pts // 2


def test_seam_helpers():
    assert chunk_seams(13, 5) == [0, 4, 5, 9, 10, 12]
    assert chunk_seams(13, 13) == chunk_seams(13, 64) == [0, 12]
    assert chunk_seams(4, 1) == [0, 1, 2, 3]
    assert time_chunk_seams(13, 5) == [0, 2, 4, 5, 7, 9, 10, 12]            # from the end: 12 7 2 (and 0)
    assert time_chunk_seams(13, 4) == [0, 3, 4, 7, 8, 11, 12] and time_chunk_seams(13, 64) == [0, 12]
    assert lane_seams(13, (4, 6)) == [3, 4, 5, 6, 7, 8, 11, 12]             # 4 8 12 | 6 12 | 11 7 3 | 11 5
    assert lane_seams(34, (16,)) == [16, 32]                                # (32 = 34 - 2 as well)
    t, counts, y_rows = pad_rows([np.array([0, 3]), np.array([1])], 3, 2)
    assert t.tolist() == [[0, 3, -1], [1, -1, -1]] and counts.tolist() == [2, 1] and counts.dtype == np.int32
    y = y_rows([np.ones((2, 2)), np.zeros((1, 2))])
    assert y.shape == (2, 3, 2) and np.isnan(y[0, 2]).all() and np.isnan(y[1, 1:]).all() and not np.isnan(y[0, :2]).any()


def _library():
    try:
        import vgpa_amd
        return vgpa_amd.load()
    except (RuntimeError, OSError):
        return None


@pytest.mark.parametrize("n_pts,world", [(13, 3), (11, 2), (10, 4), (13, 1), (3, 4), (260, 8)])
def test_rank_seams_are_the_real_slice_edges(n_pts, world):
    """The seams the sharded GPU tests place observations on are the edges vgpa_time_slice hands out (through the library when it
    loads without a device; the host formula it mirrors is checked for tiling and balance either way)."""
    lib = _library()
    edges, nxt = set(), 0
    for rank in range(world):
        lo, hi = time_slice(n_pts, rank, world)
        if lib is not None:
            a, b = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.vgpa_time_slice(n_pts, rank, world, ctypes.byref(a), ctypes.byref(b)) == 0
            assert (a.value, b.value) == (lo, hi)
        assert lo == nxt and hi - lo in (n_pts // world, n_pts // world + 1)
        nxt = hi
        if hi > lo:
            edges.update((lo, hi - 1))
    assert nxt == n_pts
    assert rank_seams(n_pts, world) == sorted(edges)
    if (n_pts, world) == (13, 3):
        assert rank_seams(n_pts, world) == [0, 4, 5, 8, 9, 12]              # slices [0, 5) [5, 9) [9, 13)
    if lib is not None:
        a, b = ctypes.c_int(), ctypes.c_int()
        assert lib.vgpa_time_slice(n_pts, world, world, ctypes.byref(a), ctypes.byref(b)) == -1


def _problem(model, pattern, n_pts=13):
    from test_gpu_edge_cases import make_problem
    d = {"OU": 1, "DW": 1, "L63": 3, "L96": 12}[model]
    return make_problem(model, d, n_pts, method="rk4", obs_at=patterns(n_pts, SEAMS_13)[pattern])


@pytest.mark.parametrize("pattern", NAMES)
@pytest.mark.parametrize("model", ["OU", "DW", "L63", "L96"])
def test_oracle_modes_agree_on_every_pattern(model, pattern):
    """Faithful (the reference's literal expressions) against lean (what the GPU tests compare with): F, gradient, lam_t, Psi_t and
    E_obs at 1e-12 in rel_err's norm -- the reference side of every GPU comparison exists for every placement."""
    p, x = _problem(model, pattern)
    f_f, g_f, s_f = vo.sweep(p, x, faithful=True)
    f_l, g_l, s_l = vo.sweep(p, x, faithful=False)
    assert np.isfinite(f_f) and np.all(np.isfinite(g_f))
    assert abs(f_f - f_l) <= 1e-12 * abs(f_f)
    assert rel_err(g_l, g_f) < 1e-12
    assert rel_err(s_l["lamt"], s_f["lamt"]) < 1e-12 and rel_err(s_l["psit"], s_f["psit"]) < 1e-12
    assert abs(s_l["Eobs"] - s_f["Eobs"]) <= 1e-12 * abs(s_f["Eobs"])


@pytest.mark.parametrize("model", ["OU", "L63", "L96"])
def test_a_lost_doubled_or_shifted_jump_is_far_above_the_tolerance(model):
    """What the GPU tests rely on: a jump that is lost (one observation dropped), doubled (one vector and matrix jump of the backward
    recursion applied twice) or shifted (one observation moved to the neighbouring grid point), and Q4's covariance diagonal read at
    t_n instead of n, each move F or the gradient by far more than the 1e-9 the GPU tests assert."""
    import dataclasses
    p, x = _problem(model, "late")
    f, g, st = vo.sweep(p, x, faithful=False)
    lost = dataclasses.replace(p, obs_t=p.obs_t[:-1], obs_y=p.obs_y[:-1])
    assert abs(vo.sweep(lost, x, faithful=False)[0] - f) > 1e-5 * abs(f)
    t_moved = p.obs_t.copy()
    t_moved[0] -= 1                                       # (`late` starts in the middle of the grid: the neighbour is free)
    f_s, g_s, _ = vo.sweep(dataclasses.replace(p, obs_t=t_moved), x, faithful=False)
    assert abs(f_s - f) > 1e-7 * abs(f) and rel_err(g_s, g) > 1e-5
    # doubled: F does not depend on the backward recursion; the gradient does
    a, _ = p.split(x)
    jm, js = vo.eobs_gradients(p, st["mt"], st["st"])
    t_mid = int(p.obs_t[1])
    jm[t_mid] *= 2.0
    js[t_mid] *= 2.0
    lam, psi = vo.solve_bwd(p.method, p.dt, p.single_dim, a, st["dEsde_dm"], st["dEsde_ds"], jm, js)
    g_d = vo.gradient(p, x, dict(st, lamt=lam, psit=psi))
    assert rel_err(g_d, g) > 1e-5
    if model != "OU":                       # Q4 (n-D only): S at the counter n, not at t_n -- `late` keeps them apart
        s_diag = np.diagonal(st["st"], axis1=1, axis2=2)
        rinv = 1.0 / np.diag(p.obs_noise)
        at_n = sum(np.inner(rinv, s_diag[n]) for n in range(p.obs_t.size))
        at_tn = sum(np.inner(rinv, s_diag[t]) for t in p.obs_t)
        assert abs(0.5 * (at_n - at_tn)) > 1e-7 * abs(f)


@pytest.mark.parametrize("tag,pattern", [("l63_rk4_every_p", "every"), ("l63_rk4_late_p", "late"), ("l96d12_rk4_every_p", "every"),
                                         ("l96d12_rk4_late_p", "late")])
def test_reference_pins_of_dense_and_late_observations(tag, pattern):
    """The four fixtures tools/gen_golden.py dumped from the reference at explicit observation indices: they hold the pattern they
    are named after, and the oracle reproduces the reference's numbers on them (F, gradient, lam_t, Psi_t, E_obs)."""
    z = load_golden(tag)
    n_pts = int(z["time_window"].size)
    assert n_pts == 13
    assert np.array_equal(z["obs_t"], patterns(n_pts)[pattern]) and np.array_equal(z["obs_at"], z["obs_t"])
    assert z["obs_y"].shape[0] == z["obs_t"].size
    p = vo.Problem.from_fixture(z)
    f, g, st = vo.sweep(p, z["x"], faithful=True)
    assert abs(f - float(z["F"])) <= 1e-12 * abs(float(z["F"]))
    assert rel_err(g, z["grad"]) < 1e-12
    assert rel_err(st["lamt"], z["lamt"]) < 1e-12 and rel_err(st["psit"], z["psit"]) < 1e-12
    assert abs(st["Eobs"] - float(z["Eobs"])) <= 1e-12 * abs(float(z["Eobs"]))
