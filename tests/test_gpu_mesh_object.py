"""GPU (-m gpu): what the four objects built on a mesh and a caller's hierarchy hold in HBM (csrc/smg_mesh_object.hpp).  Per object: create,
use once, read device_bytes() and the library's count of live DevBuf bytes, destroy.  Everything device_bytes() counts is a live buffer and
nothing is counted twice, and the teardown -- which names no buffer -- gives every byte back."""
import gc

import numpy as np
import pytest

from test_arap_host import twist
from test_geodesics_host import icosphere
from test_gpu_parity import smg  # noqa: F401  (fixture)
from problems import subdiv_problem
from test_membrane_host import load_mesh

pytestmark = pytest.mark.gpu


def _geodesics(smg):
    V, F = icosphere(3)
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    return mg, lambda: smg.HeatGeodesics(mg, V, F), lambda g: g.distance([0, [5, 100, 641]])


def _arap(smg):
    V, F = icosphere(3)
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    handles, hp = twist(V)
    return mg, lambda: smg.ArapDeformer(mg, V, F, handles), lambda a: a.deform(hp, max_iter=2)


def _membrane(smg):
    V, F = load_mesh("ogre_sim.smgm")
    mg = smg.mg_precompute_block(V, F)
    return mg, lambda: smg.MembraneSim(mg, V, F, newton_iters=2), lambda m: m.step()


def _param(smg):
    V, F = load_mesh("ogre_sim.smgm")                                              # 2 612 vertices, a disk
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    return mg, lambda: smg.Parameterizer(mg, V, F), lambda p: p.distortion(p.flatten(max_iter=2)[0])


@pytest.mark.parametrize("which", ["geodesics", "arap", "membrane", "param"])
def test_device_bytes_are_live_buffers_and_destroy_frees_them(smg, which):
    live = smg._lib.load().smg_device_bytes_live
    mg, create, use = {"geodesics": _geodesics, "arap": _arap, "membrane": _membrane, "param": _param}[which](smg)    # the caller's hierarchy stays alive throughout
    gc.collect()
    before = live()
    obj = create()
    use(obj)
    counted, held = obj.device_bytes(), live() - before
    print("%s: device_bytes %d, live DevBuf bytes held %d, difference %d" % (which, counted, held, held - counted))
    del obj
    gc.collect()
    after = live()
    assert 0 < counted == held
    assert after == before
    assert mg.n_levels >= 2


def test_a_hierarchy_reports_the_bytes_it_holds_after_a_mixed_solve(smg):
    """a plain hierarchy handle after an fp64 and a mixed-precision solve -- the fp32 images of its matrices and the fp32 vectors exist --
    reports, line by line, what it holds: the total of device_bytes() is the growth of the library's count of live DevBuf bytes since before
    the handle was created, and destroying the handle gives every byte back"""
    live = smg._lib.load().smg_device_bytes_live
    p = subdiv_problem(kind="mcf", k=2, n_sub=2)
    gc.collect()
    before = live()
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"])
    for precision in ("f64", "mixed"):
        assert mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-8, max_iter=30, precision=precision))[0]
    rep = mg.device_bytes()
    held = live() - before
    print("hierarchy: total %d, live DevBuf bytes held %d; fp32 images %d" % (rep["total"], held, sum(v for k, v in rep.items() if k.endswith("fp32_images"))))
    assert 0 < rep["total"] == held
    assert rep["total"] == sum(v for k, v in rep.items() if k != "total")
    assert all(rep.get("level%d.fp32_images" % lv, 0) > 0 for lv in range(mg.n_levels - 1))
    del mg
    gc.collect()
    assert live() == before
