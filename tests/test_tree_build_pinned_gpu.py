"""The device tree builders, pinned: the node bytes every build path writes - the forest at scene load, hk_rebuild_mesh_tree, and
hk_rebuild_scene_trees for the instance tree and the light tree - in both tree modes and both traversal settings, against the digests
recorded in tests/golden/tree_build_digests.json.  The SAH trees are also held to the host builder elsewhere (test_mesh_rebuild_gpu.py,
test_scene_load_gpu.py, test_device_refit.py); the Morton-order trees are only checked for validity there, so their bytes are pinned
here.  The sizes are the smallest at which each path can go wrong: 1, 2 and 3 triangles, either side of the subtree size (1024 / 1025),
a grid of about 3000, a mesh whose triangles share one centre (equal Morton codes, the SAH half cut) and the first size that leaves the
forest for the multi-workgroup top (32768).  The fixture is only read here.
A gap: the instance tree and the light tree are read through hk_debug_read_trees, which returns ordering 0 alone.  The 'threaded' cases
of test_rebuild_trees_* therefore pin the same bytes as the 'reference' ones; orderings 1-7 of a threaded instance tree are not pinned
here (the mesh trees, read through hk_debug_read_mesh_nodes, are pinned in all eight)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from cases import product_default_traversal
from conftest import ROOT
from test_mesh_rebuild import IDENTITY, NODE, flat, half_split_mesh
from test_mesh_rebuild_gpu import SIZED, soup

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_build_digests.json")
MODES = {"lbvh": F.TREE_LBVH, "sah": F.TREE_SAH}
TREES = [(1, 0), (1, 1), (2, 2), (1500, 40)]   # (instances, emitters)


def plugin(threaded):
    if threaded:
        with product_default_traversal():
            return hk.HikariPlugin(device=0, flags=0)
    return hk.HikariPlugin(device=0)


def digest(raw, fold_zero=False):
    """sha256 of node bytes; fold_zero: every box bound of -0 counted as +0"""
    a = np.frombuffer(bytes(raw), NODE).copy()
    if fold_zero:
        for f in ("min", "max"):
            a[f][a[f] == 0] = 0.0
    return hashlib.sha256(a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def mesh_inputs():
    """name -> (positions, indices), in the order they are added (made at the first use, not at import)"""
    out = {k: (SIZED[k][0], SIZED[k][2]) for k in ("1", "2", "3", "1024", "1025")}
    p, _, _, idx = S.cloth_grid(39, 39, size=2.0)   # 3042 triangles
    out["grid_3042"] = (p, idx)
    out["one_centre_300"] = half_split_mesh(300)
    p, _, idx = soup(32768, 32768)
    out["32768"] = (p, idx)
    return out


def mesh_builder(names, deferred):
    """one instance of each named mesh: (finished builder, {name: mesh id})"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    ids = {}
    for name in names:
        p, idx = mesh_inputs()[name]
        n, uv = flat(p)
        ids[name] = b.add_mesh(p, n, uv, idx, build_tree=not deferred)
        b.add_instance(ids[name], mat, IDENTITY)
    b.finish()
    return b, ids


def load_case(mode, threaded):
    """every mesh deferred, built by hk_load_scene: (plugin, builder, ids, record)"""
    b, ids = mesh_builder(list(mesh_inputs()), deferred=True)
    gpu = plugin(threaded)
    gpu.load_scene(b, MODES[mode])
    raw, count, orderings = gpu.engine.read_mesh_nodes()
    meshes, tris, launches, on_host = gpu.engine.last_load()
    assert (meshes, on_host) == (len(mesh_inputs()), 0)
    return gpu, b, ids, {"raw": raw, "count": count, "orderings": orderings, "launches": launches}


def rebuild_case(mode, threaded):
    names = ["2", "1025", "32768"]
    b, ids = mesh_builder(names, deferred=False)
    gpu = plugin(threaded)
    gpu.set_scene(b.scene())
    for name in names:
        gpu.engine.rebuild_mesh_tree(b.mesh_index(ids[name]), MODES[mode])
    raw, count, orderings = gpu.engine.read_mesh_nodes()
    return {"raw": raw, "count": count, "orderings": orderings}


def instance_scene(n_instances, n_emitters):
    """n_instances poses of one quad drawn from a fixed seed, the first n_emitters of them glowing"""
    rng = np.random.default_rng(1000 * n_instances + n_emitters)
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    p, n, uv, idx = S.cloth_grid(1, 1, size=0.5)
    mesh = b.add_mesh(p, n, uv, idx)
    for k in range(n_instances):
        pose = S._trs(rng.uniform(-8.0, 8.0, 3), rng.uniform(-3.0, 3.0, 3), rng.uniform(0.5, 2.0, 3))
        b.add_instance(mesh, glow if k < n_emitters else mat, pose)
    return b.finish()


def trees_case(n_instances, n_emitters, mode, threaded):
    scene = instance_scene(n_instances, n_emitters)
    assert len(scene.instances) == n_instances and len(scene.emissives) == n_emitters
    gpu = plugin(threaded)
    gpu.set_scene(scene)
    gpu.engine.rebuild_trees(MODES[mode])
    tlas, light = gpu.engine.read_trees(len(scene.instance_nodes), len(scene.emissive_nodes))
    return {"raw": bytes(tlas) + bytes(light), "count": len(scene.instance_nodes) + len(scene.emissive_nodes), "orderings": 1}


def case_id(kind, mode, threaded):
    return f"{kind}[{mode},{'threaded' if threaded else 'reference'}]"


def compare(name, got):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][name]
    fold = bool(want.get("fold_zero", False))
    rec = {"sha256": digest(got["raw"], fold), "count": got["count"], "orderings": got["orderings"]}
    if "launches" in got:
        rec["launches"] = got["launches"]
    print(name, rec)
    assert rec == {k: want[k] for k in rec}, f"{name}: the node bytes (or their count, or the launches) differ from the pinned build"


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("mode", ["lbvh", "sah"])
def test_load_scene_builds_the_pinned_mesh_trees(mode, threaded):
    compare(case_id("load", mode, threaded), load_case(mode, threaded)[3])


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("mode", ["lbvh", "sah"])
def test_rebuild_mesh_tree_builds_the_pinned_mesh_trees(mode, threaded):
    compare(case_id("rebuild", mode, threaded), rebuild_case(mode, threaded))


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("mode", ["lbvh", "sah"])
@pytest.mark.parametrize("n_instances,n_emitters", TREES)
def test_rebuild_trees_builds_the_pinned_instance_and_light_trees(n_instances, n_emitters, mode, threaded):
    compare(case_id(f"trees_{n_instances}_{n_emitters}", mode, threaded), trees_case(n_instances, n_emitters, mode, threaded))


@pytest.mark.parametrize("threaded", [False, True])
def test_the_forest_and_the_single_tree_build_agree_in_lbvh_mode(threaded):
    """The two paths share every construction step: a mesh built by the forest (or, at 32768 triangles, beside it) at load and then
    rebuilt, undeformed, by hk_rebuild_mesh_tree keeps its node bytes."""
    gpu, b, ids, rec = load_case("lbvh", threaded)
    loaded = bytes(rec["raw"])
    for name, mesh in ids.items():
        gpu.engine.rebuild_mesh_tree(b.mesh_index(mesh), F.TREE_LBVH)
        again = bytes(gpu.engine.read_mesh_nodes()[0])
        assert again == loaded, f"mesh {name}: the rebuilt Morton-order tree differs from the one the load built"
