"""
Observation placements for the tests: the ONLY place a pattern is spelled.

Every backward recursion, every observation kernel and every E_obs sum takes its jumps from the observation set; the equidistant sets
of the other tests (every fifth grid point from 2 on) never put two observations next to each other, never observe the last grid
point and never let the counter n of an observation (quirk Q4: the covariance diagonal of observation n is read at grid index n, not
at t_n) leave the first few grid points.  `patterns` names the placements that do.
"""
import numpy as np

NAMES = ("every", "inner", "ends", "head", "tail", "run", "late", "seams")


def expected_count(name, n_pts):
    """M of pattern `name` on a grid of n_pts points; None where the grid is too short for it (`patterns` then leaves it out).
    `seams` depends on the caller's seams and is not listed."""
    n = int(n_pts)
    return {"every": n, "inner": n - 2 if n >= 3 else None, "ends": 2 if n >= 2 else None, "head": 3 if n >= 3 else None,
            "tail": 3 if n >= 3 else None, "run": 4 if n >= 8 else None, "late": (n + 1) // 2}[name]


def patterns(n_pts, seams=()):
    """name -> sorted int64 grid indices, strictly increasing, inside [0, n_pts):
      every   0 ... Np-1 (M = Np: a jump on every step, Q4's n reaches the last grid point)
      inner   1 ... Np-2
      ends    0, Np-1
      head    the first three grid points          tail    the last three
      run     2, 3, 4 and the isolated point Np-2 (Np >= 8, so that it touches neither the run nor the end)
      late    the last ceil(Np / 2) points: n and t_n of one observation lie far apart
      seams   s-1, s, s+1 for every seam s the caller names, clipped to the grid and deduplicated (only with seams)
    A pattern the grid is too short for is left out (expected_count: None)."""
    n = int(n_pts)
    assert n >= 2
    out = {"every": np.arange(n)}
    if n >= 3:
        out["inner"] = np.arange(1, n - 1)
    out["ends"] = np.array([0, n - 1])
    if n >= 3:
        out["head"], out["tail"] = np.arange(3), np.arange(n - 3, n)
    if n >= 8:
        out["run"] = np.array([2, 3, 4, n - 2])
    out["late"] = np.arange(n - (n + 1) // 2, n)
    seams = [int(s) for s in seams]
    if seams:
        out["seams"] = np.array(sorted({t for s in seams for t in (s - 1, s, s + 1) if 0 <= t < n}))
    return {k: np.asarray(v, dtype=np.int64) for k, v in out.items()}


def time_slice(n_pts, rank, world):
    """[t_lo, t_hi) of `rank`: the host formula of vgpa_time_slice (the first Np mod world ranks own one grid point more)."""
    base, rem = n_pts // world, n_pts % world
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def rank_seams(n_pts, world):
    """t_lo and t_hi - 1 of every rank that owns a grid point"""
    out = set()
    for rank in range(world):
        lo, hi = time_slice(n_pts, rank, world)
        if hi > lo:
            out.update((lo, hi - 1))
    return sorted(out)


def chunk_seams(n_pts, chunk):
    """first and last grid point of every chunk of `chunk` points counted from the grid's start"""
    return sorted({t for lo in range(0, n_pts, chunk) for t in (lo, min(lo + chunk, n_pts) - 1)})


def time_chunk_seams(n_pts, chunk):
    """The chunk edges of the time-chunked D > 64 sweep (VGPA_OPT_LD_CHUNK = chunk): it walks the grid from its END in chunks
    [t1 - chunk, t1] that share their edge point, t1 = Np - 1, Np - 1 - chunk, ...  The edges counted from the grid's start
    (k chunk) are seams of no kernel; they are included for margin only."""
    return sorted(set(chunk_seams(n_pts, chunk)) | set(range(n_pts - 1, 0, -chunk)) | {0})


def lane_seams(n_pts, sizes):
    """The chunk boundaries of the lane kernels for the chunk sizes `sizes` (forward kernel TT, fused pass T).  The forward kernel's
    chunk c holds the grid points [c T + 1, c T + T], the forward half of the pass [c T, c T + T), the backward half
    [hi - T + 1, hi] with hi = Np - 2 - c T: multiples of T from the start, and Np - 2 - k T from the end."""
    out = set()
    for t in sizes:
        out.update(range(t, n_pts, t))
        out.update(range(n_pts - 2, 0, -t))
    return sorted(s for s in out if 0 < s < n_pts)


def pad_rows(rows, capacity, d):
    """Per-problem observation rows of one capacity: (obs_t (B, M) padded with -1, n_obs (B,)), and for obs_y a function
    y_rows(list of (M_k, d) arrays) -> (B, M, d) padded with NaN."""
    b = len(rows)
    t = np.full((b, capacity), -1, dtype=np.int64)
    for k, r in enumerate(rows):
        t[k, :len(r)] = r
    counts = np.array([len(r) for r in rows], dtype=np.int32)

    def y_rows(ys):
        y = np.full((b, capacity, d), np.nan)
        for k, v in enumerate(ys):
            y[k, :len(v)] = np.reshape(v, (len(v), d))
        return y
    return t, counts, y_rows
