"""GPU (-m gpu): examples/06_balloon_sim.cpp -- the reference's 06_example_balloon_sim/main.cpp on the C++ mirror (mg_precompute_block,
balloon_sim_precompute, implicit_euler_mg_balloon of csrc/mg_api.hpp) -- against the python path on the same mesh."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_api import ROOT, _stale

pytestmark = pytest.mark.gpu


def test_cpp_balloon_example_matches_python_path(smg_mod):
    smg = smg_mod
    exe = os.path.join(ROOT, "examples", "06_balloon_sim")
    src = os.path.join(ROOT, "examples", "06_balloon_sim.cpp")
    lib = os.path.join(ROOT, "surface_multigrid_code_amd", "lib")
    if _stale(exe, [src]):
        subprocess.check_call(["hipcc", "-std=c++17", "-O2", src, "-L" + lib, "-lsmg", "-Wl,-rpath," + lib, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.check_output([exe, os.path.join(ROOT, "tests", "golden", "meshes", "bunny_15K_init.smgm"), "2"], env=env, text=True)
    rows = re.findall(r"newton (\d+): objective ([0-9.eE+-]+) alpha: ([0-9.eE+-]+) cycles: (\d+)", out)
    ends = re.findall(r"step (\d+): objective ([0-9.eE+-]+) max displacement ([0-9.eE+-]+)", out)
    assert len(rows) == 20 and len(ends) == 2
    V, F = smg.mesh.read_triangle_mesh("bunny_15K_init.smgm")
    sim = smg.MembraneSim(smg.mg_precompute_block(V, F), V, F)
    for k in range(2):
        r = sim.step()
        got = rows[10 * k:10 * k + 10]
        assert [int(x[3]) for x in got] == list(r["cycles"]) and [float(x[2]) for x in got] == list(r["alpha"])
        np.testing.assert_allclose([float(x[1]) for x in got], r["objective"][:10], rtol=1e-14)       # printed with %.15g
        assert abs(float(ends[k][1]) - r["objective"][10]) <= 1e-14 * abs(r["objective"][10])
        assert abs(float(ends[k][2]) - np.abs(sim.state()[0] - V).max()) <= 1e-6 * float(ends[k][2])
