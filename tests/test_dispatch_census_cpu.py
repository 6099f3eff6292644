"""
Which kernel every launcher picks, with what grid, block and dynamic LDS, over the whole run-time domain of its request: the output of
tools/host_check/dispatch_census.cpp -- the host code of the launcher files linked against a recording HIP runtime, run on the CPU -- held to
tests/golden/dispatch_census.txt.  No device: a launcher that picks another kernel, another shape or another return code for any request
changes its family's hash, one that opts in to dynamic LDS elsewhere the hash of its opt-ins; the program's --outcomes then says where.
(The address / undefined-behaviour sanitizer build is the manual line at the head of the tool and prints the same text; this test builds
without the sanitizers and links with the system's c++, so that it needs no sanitizer runtime where it runs.)
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vgpa_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "host_check", "dispatch_census.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_census.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LAUNCHER_FILES = ["ode_generic", "ode_small", "ode_wave", "ode_mfma", "ode_mfma_m0", "ode_mfma_m1", "ode_mfma_m2", "ode_mfma_m3", "energy", "assemble",
                  "lag_cov", "sample", "large_d", "large_d_stage", "large_d_energy"]


def _compile(src, obj):
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-4000:]}"
    return obj


def test_dispatch_census_matches_golden(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip(f"hipcc not found ({HIPCC}): the dispatch census compiles the launcher files' host code with it")
    jobs = [(os.path.join(CSRC, f + ".hip"), str(tmp_path / (f + ".o"))) for f in LAUNCHER_FILES] + [(TOOL, str(tmp_path / "dispatch_census.o"))]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(lambda j: _compile(*j), jobs))
    exe = str(tmp_path / "dispatch_census")
    # (the launchers of the other files and the rest of the HIP runtime stay unresolved and are never called)
    link = subprocess.run([shutil.which("c++") or "g++", *objs, "-Wl,--unresolved-symbols=ignore-all", "-o", exe], capture_output=True, text=True)
    assert link.returncode == 0, link.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    got, want = run.stdout.splitlines(), open(GOLDEN).read().splitlines()
    diff = [f"line {i + 1}:\n  golden: {w[:300]}\n  now:    {g[:300]}" for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, f"{len(got)} lines against the golden file's {len(want)}; first differences:\n" + "\n".join(diff[:10])
    assert "registered, never launched, not excused: 0" in got, "a kernel of a launcher file is launched by no request: add the request (or the reason)"
    assert run.returncode == 0, run.stderr[-2000:]
