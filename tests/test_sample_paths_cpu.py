"""
Sample paths (vgpa_sample_paths): the numpy restatement of the generator and of the Euler-Maruyama recursion, and the host-side surface.

The restatement is the reference of tests/test_sample_paths.py: Philox4x32-10 -> two uniforms of 53 bits -> Box-Muller, counter
(grid index, path, problem, component pair), key (seed & 0xffffffff, seed >> 32); x_k = x_{k-1} + dt drift_{k-1}(x_{k-1}) + R xi_k with
R = chol_lower(Sigma dt).

u = (n + 0.5) 2^-53 of a 53-bit n lies in (0, 1) in exact arithmetic; in fp64 n + 0.5 is a tie from 2^52 on and the largest n, 2^53 - 1,
rounds up to 2^53, i.e. u = 1.  The restatement (and the kernel) cap u at 1 - 2^-53, the largest double below 1: every other n gives
the fp64 value of the formula unchanged.
"""
import os
import re

import numpy as np
import pytest

import vgpa_amd as va
from vgpa_amd import _lib
from conftest import ROOT

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
U_MAX = 1.0 - 2.0 ** -53


def philox4x32_10(counter, key):
    """counter: four uint32 words (arrays broadcast against each other), key: two words -> four uint32 arrays"""
    c = [np.asarray(w, dtype=np.uint64) & MASK for w in np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) for w in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def unit_open(hi, lo):
    n = (np.asarray(hi, dtype=np.uint64) >> np.uint64(5)) * np.uint64(1 << 26) + (np.asarray(lo, dtype=np.uint64) >> np.uint64(6))
    return np.minimum((n.astype(np.float64) + 0.5) * 2.0 ** -53, U_MAX)


def normals(seed, k, path, problem, d):
    """The d standard normals of grid index k, path `path`, problem `problem`; k and path may be arrays (broadcast): (..., d)."""
    k, path = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(path, dtype=np.uint64))
    j = np.arange((d + 1) // 2, dtype=np.uint64)
    r = philox4x32_10((k[..., None], path[..., None], np.uint64(problem), j), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1, u2 = unit_open(r[0], r[1]), unit_open(r[2], r[3])
    rho = np.sqrt(-2.0 * np.log(u1))
    z = np.stack((rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)), axis=-1)
    return z.reshape(z.shape[:-2] + (-1,))[..., :d]


def start_cloud(problem, x0, seed, words, index=0):
    """(len(words), D): the start of every walk -- m0 + chol(S0) xi_0 with the normals of grid index 0 and the counter words `words`, or
    the given x0 once per word"""
    d = int(problem.dim_d)
    if x0 is not None:
        return np.tile(np.reshape(np.asarray(x0, dtype=float), (1, d)), (len(words), 1))
    l0 = np.linalg.cholesky(np.reshape(np.asarray(problem.s0, dtype=float), (d, d)))
    return np.reshape(np.asarray(problem.m0, dtype=float), (1, d)) + normals(seed, 0, words, index, d) @ l0.T


def em_noise(seed, k, words, index, fac):
    """(len(words), D): eta_k = R xi_k of the step to grid index k, R = fac = chol(Sigma dt)"""
    return normals(seed, k, words, index, fac.shape[0]) @ fac.T


def em_step(state, dt, g, eta):
    """the Euler-Maruyama step, in the order every walk of the tests (and the device) adds it up"""
    return (state + dt * g) + eta


def n_keep(n_pts, stride):
    return (n_pts - 1) // stride + 1


def model_drift(model, theta, x):
    """x: (n_paths, D)"""
    if model == "OU":
        return -theta * x
    if model == "DW":
        return 4.0 * x * (theta - x * x)
    if model == "L63":
        s, r, b = theta
        return np.stack((s * (x[:, 1] - x[:, 0]), (r - x[:, 2]) * x[:, 0] - x[:, 1], x[:, 0] * x[:, 1] - b * x[:, 2]), axis=1)
    return (np.roll(x, -1, axis=1) - np.roll(x, 2, axis=1)) * np.roll(x, 1, axis=1) - x + theta     # dynamics.Lorenz96._drift per path


def sample_paths_numpy(problem, kind, x, x0, n_paths, stride, seed, index=0):
    """The recursion of vgpa_sample_paths for ONE problem (an oracle Problem, or anything with its fields) whose counter word is `index`:
    (n_paths, n_keep, D).  kind "posterior": x = [A_t | b_t]; "model": the model's drift at problem.theta.  x0 None: m0 + chol(S0) xi_0."""
    d, n, dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
    sigma = np.reshape(np.asarray(problem.sigma, dtype=float), (d, d))
    fac = np.linalg.cholesky(sigma * dt)
    paths = np.arange(n_paths)
    state = start_cloud(problem, x0, seed, paths, index)
    if kind == "posterior":
        x = np.asarray(x, dtype=float)
        lin_a, off_b = x[:n * d * d].reshape(n, d, d), x[n * d * d:].reshape(n, d)
    theta = np.asarray(problem.theta, dtype=float)
    out = np.empty((n_paths, n_keep(n, stride), d))
    out[:, 0] = state
    for k in range(1, n):
        if kind == "posterior":
            drift = -(state @ lin_a[k - 1].T) + off_b[k - 1]
        else:
            drift = model_drift(problem.model, theta, state)
        state = em_step(state, dt, drift, em_noise(seed, k, paths, index, fac))
        if k % stride == 0:
            out[:, k // stride] = state
    return out


def em_moments(problem, x, stride=1):
    """Mean and covariance of the Euler-Maruyama chain of the posterior kind started at N(m0, S0): (n_keep, D), (n_keep, D, D)"""
    d, n, dt = int(problem.dim_d), int(problem.n_pts), float(problem.dt)
    x = np.asarray(x, dtype=float)
    lin_a, off_b = x[:n * d * d].reshape(n, d, d), x[n * d * d:].reshape(n, d)
    sigma = np.reshape(np.asarray(problem.sigma, dtype=float), (d, d))
    m, s = np.reshape(np.asarray(problem.m0, dtype=float), d).copy(), np.reshape(np.asarray(problem.s0, dtype=float), (d, d)).copy()
    ms, ss = [m], [s]
    for k in range(1, n):
        t = np.eye(d) - dt * lin_a[k - 1]
        m, s = t @ m + dt * off_b[k - 1], t @ s @ t.T + dt * sigma
        if k % stride == 0:
            ms.append(m)
            ss.append(s)
    return np.array(ms), np.array(ss)


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == want


def test_uniforms_stay_inside_the_unit_interval():
    for word in (0, 0xFFFFFFFF):
        u = float(unit_open(word, word))
        assert 0.0 < u < 1.0, (word, u)
    assert float(unit_open(0, 0)) == 2.0 ** -54
    # every n but the largest is the fp64 value of the formula itself
    assert float(unit_open(0xFFFFFFFF, 0xFFFFFFBF)) == ((2.0 ** 53 - 2.0) + 0.5) * 2.0 ** -53


def test_normals_are_counter_based():
    z = normals(20261018, np.arange(4)[:, None], np.arange(3)[None, :], 5, 7)
    assert z.shape == (4, 3, 7) and np.all(np.isfinite(z)) and np.max(np.abs(z)) <= 8.66
    assert np.array_equal(z[2, 1], normals(20261018, 2, 1, 5, 7))
    assert np.array_equal(z[..., :6], normals(20261018, np.arange(4)[:, None], np.arange(3)[None, :], 5, 6))   # odd D drops half a pair
    assert not np.array_equal(z, normals(20261018, np.arange(4)[:, None], np.arange(3)[None, :], 6, 7))
    assert not np.array_equal(z, normals(20261018 + (1 << 32), np.arange(4)[:, None], np.arange(3)[None, :], 5, 7))
    big = normals(7, np.arange(2000)[:, None], np.arange(50)[None, :], 0, 2).ravel()
    assert abs(big.mean()) < 4.5 / np.sqrt(big.size) and abs(big.var() - 1.0) < 4.5 * np.sqrt(2.0 / big.size)


@pytest.mark.parametrize("n_pts,stride,want", [(51, 1, 51), (51, 4, 13), (51, 50, 2), (51, 51, 1), (2, 1, 2)])
def test_n_keep(n_pts, stride, want):
    assert n_keep(n_pts, stride) == want == len(range(0, n_pts, stride))


def test_numpy_recursion_on_a_linear_problem():
    """OU model kind against the closed form of its Euler-Maruyama chain, and the posterior kind with A = theta, b = 0 against the model kind"""
    class P:
        model, dim_d, n_pts, dt, theta, sigma, m0, s0 = "OU", 1, 9, 0.01, 2.0, 0.5, 0.3, 0.2
    got = sample_paths_numpy(P, "model", None, [0.7], 3, 2, 11)
    assert got.shape == (3, 5, 1)
    xi = normals(11, np.arange(9)[:, None], np.arange(3)[None, :], 0, 1)[..., 0]
    want = np.full(3, 0.7)
    for k in range(1, 9):
        want = want * (1.0 - 0.01 * 2.0) + np.sqrt(0.5 * 0.01) * xi[k]
        if k % 2 == 0:
            assert np.allclose(got[:, k // 2, 0], want, rtol=1e-14, atol=0.0)
    x = np.concatenate((np.full(9, 2.0), np.zeros(9)))
    assert np.allclose(sample_paths_numpy(P, "posterior", x, [0.7], 3, 2, 11), got, rtol=1e-14, atol=0.0)
    drawn = sample_paths_numpy(P, "posterior", x, None, 3, 9, 11)
    assert drawn.shape == (3, 1, 1) and np.allclose(drawn[:, 0, 0], 0.3 + np.sqrt(0.2) * xi[0], rtol=1e-14, atol=0.0)


def test_symbol_and_prototype():
    assert "vgpa_sample_paths" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "vgpa_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+VGPA_ABI_VERSION\s+2\b", header)
    assert _lib.ABI_VERSION == 2
    proto = re.search(r"int\s+vgpa_sample_paths\s*\(([^;]*)\)\s*;", header)
    assert proto, "prototype missing"
    args = " ".join(proto.group(1).split())
    assert args == ("vgpa_ctx* ctx, int kind, const double* x_or_null, const double* x0_or_null, int32_t n_paths, int32_t stride, "
                    "uint64_t seed, double* out")
    assert re.search(r"enum\s*\{\s*VGPA_PATHS_POSTERIOR\s*=\s*0\s*,\s*VGPA_PATHS_MODEL\s*=\s*1\s*\}", header)
    assert _lib.PATH_KINDS == {"posterior": 0, "model": 1}


def test_python_surface():
    import inspect
    for owner, name, params in [(va.Context, "sample_paths", ["kind", "n_paths", "seed", "stride", "x", "x0"]),
                                (va.VarGP, "sample_paths", ["n_paths", "seed", "stride", "x", "x0"]),
                                (va.ProblemBatch, "sample_paths", ["n_paths", "seed", "stride", "x", "x0"]),
                                (va.StochasticProcess, "sample_trajectories", ["x0", "n_paths", "t0", "tf", "dt", "seed", "stride"])]:
        fn = getattr(owner, name, None)
        assert callable(fn), (owner.__name__, name)
        got = list(inspect.signature(fn).parameters)[1:]
        assert got[:len(params)] == params, (owner.__name__, name, got)
