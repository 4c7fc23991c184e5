"""Deferred meshes on the host (hk_scene_builder_add_mesh_deferred / _pending_mesh_trees / _build_pending_mesh_trees): a mesh added
without its tree carries a valid stand-in of the final size, and the host completion gives, in place, the arrays of the twin builder
(add_mesh + hk_scene_builder_rebuild_mesh_tree) - every buffer byte for byte.  hk_load_scene builds the same trees on the device
(tests/test_scene_load_gpu.py).  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from test_mesh_rebuild import IDENTITY, NODE, flat, half_split_mesh, node_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0x80000000
BUFFERS = ("vertices", "primitives", "asset_nodes", "materials", "instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table")


def soup(k, seed):
    """k small separate triangles in a box"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (k, 1, 3))
    return (c + rng.uniform(-0.05, 0.05, (k, 3, 3))).reshape(-1, 3).astype(np.float32), np.arange(3 * k, dtype=np.uint32), F.TOPOLOGY_TRIANGLE_LIST


def strip(k=41):
    """a triangle strip of k triangles that winds through space (odd triangles flip their winding in the builder)"""
    t = np.arange(k + 2, dtype=np.float32)
    p = np.stack([0.1 * t, 0.3 * np.sin(0.7 * t) + 0.2 * (t % 2), 0.25 * np.cos(0.4 * t)], 1).astype(np.float32)
    return p, np.arange(k + 2, dtype=np.uint32), F.TOPOLOGY_TRIANGLE_STRIP


def signed_zero_grid(n=64):
    """an n x n grid in the plane y = 0 whose y coordinates mix +0 and -0: add_mesh keeps the first zero it meets in a navigator box,
    the canonical union has -0 < +0 - the contract is the add_mesh + rebuild_mesh_tree twin, not raw add_mesh"""
    p, _, _, idx = S.cloth_grid(n, n, size=2.0)
    p = p.copy()
    p[:, 1] = np.where((np.arange(len(p)) * 7 + 3) % 5 < 2, np.float32(-0.0), np.float32(0.0))
    return p.astype(np.float32), idx, F.TOPOLOGY_TRIANGLE_LIST


def meshes():
    out = {f"soup_{k}": soup(k, k) for k in (1, 2, 3, 1023, 1024, 1025)}
    hp, hidx = half_split_mesh(2500)
    out["half_split"] = (hp, hidx, F.TOPOLOGY_TRIANGLE_LIST)
    out["strip"] = strip()
    out["signed_zero_grid"] = signed_zero_grid()
    return out


MESHES = meshes()
SOUPS = tuple(n for n in MESHES if n.startswith("soup_"))


def builder_with(name, how):
    """[a bystander cloth, the mesh under test, a bystander sphere], one instance each and an emitter; how: 'plain' (add_mesh), 'twin'
    (add_mesh + rebuild_mesh_tree) or 'deferred'"""
    p, idx, topology = MESHES[name]
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    cp, cn, cuv, ci = S.cloth_grid(5, 4)
    ids = [b.add_mesh(cp, cn, cuv, ci)]
    n, uv = flat(p)
    mesh = b.add_mesh(p, n, uv, idx, topology, build_tree=how != "deferred")
    if how == "twin":
        b.rebuild_mesh_tree(mesh)
    ids.append(mesh)
    sp, sn, suv, si = S._sphere(5, 6)
    ids.append(b.add_mesh(sp, sn, suv, si))
    for k, m in enumerate(ids):
        b.add_instance(m, glow if k == 2 else mat, IDENTITY)
    return b, mesh


def buffers(scene):
    return {n: bytes(getattr(scene, n)) for n in BUFFERS}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_deferred_then_host_completion_equals_the_twin_builder(name):
    d, mesh = builder_with(name, "deferred")
    assert d.pending_mesh_trees() == 1
    standin = d.finish()
    assert d.pending_mesh_trees() == 1
    index = d.mesh_index(mesh)
    d.build_pending_mesh_trees()
    assert d.pending_mesh_trees() == 0
    got = d.scene()   # (no second finish: the completion is in place)
    t, tmesh = builder_with(name, "twin")
    want = t.finish()
    tindex = t.mesh_index(tmesh)
    assert bytes(index) == bytes(tindex), "mesh_index was not final before the build"
    for n in BUFFERS:
        assert bytes(getattr(got, n)) == bytes(getattr(want, n)), f"{name}: {n} differs from the add_mesh + rebuild_mesh_tree twin's"
    # everything but the mesh's own nodes was final with the stand-in
    lo, hi = index.node_offset, index.node_offset + index.node_count
    a, s = node_array(got.asset_nodes), node_array(standin.asset_nodes)
    assert a[:lo].tobytes() == s[:lo].tobytes() and a[hi:].tobytes() == s[hi:].tobytes()
    for n in BUFFERS:
        if n != "asset_nodes":
            assert bytes(getattr(standin, n)) == bytes(getattr(want, n)), n
    # a later finish keeps the completed tree
    assert buffers(d.finish())["asset_nodes"] == bytes(want.asset_nodes)
    if name in SOUPS:   # (no box face holds both zeros: the canonical form is add_mesh's own)
        p, _ = builder_with(name, "plain")
        plain = p.finish()
        for n in BUFFERS:
            assert bytes(getattr(got, n)) == bytes(getattr(plain, n)), f"{name}: {n} differs from plain add_mesh"


def test_signed_zero_grid_differs_from_plain_add_mesh_only_in_the_sign_of_zeros():
    d, mesh = builder_with("signed_zero_grid", "deferred")
    d.finish()
    d.build_pending_mesh_trees()
    p, _ = builder_with("signed_zero_grid", "plain")
    a, b = node_array(d.scene().asset_nodes), node_array(p.finish().asset_nodes)
    assert np.array_equal(a["entry"], b["entry"]) and np.array_equal(a["exit"], b["exit"])
    assert np.array_equal(a["min"], b["min"]) and np.array_equal(a["max"], b["max"])   # (by value)
    assert a.tobytes() != b.tobytes(), "the fixture no longer tells the canonical union from add_mesh's"


@pytest.mark.parametrize("name", sorted(MESHES))
def test_standin_tree_is_valid(name):
    """3n - 2 nodes in the flatten_custom layout, every triangle reachable exactly once by the skip-link walk, every navigator box the
    union of the triangle boxes of its range"""
    d, mesh = builder_with(name, "deferred")
    scene = d.finish()
    i = d.mesh_index(mesh)
    prims = np.frombuffer(bytes(scene.primitives), np.dtype([("v", [("p", "<f4", 3), ("i", "<u4")], 3)]))["v"]["p"][i.primitive:]
    a = node_array(scene.asset_nodes)[i.node_offset:i.node_offset + i.node_count]
    leaf = a["entry"] >= LEAF
    n_tris = int(leaf.sum())
    assert len(a) == 3 * n_tris - 2
    seen, k, steps = [], 0, 0
    while k < len(a):   # the walk of a ray that hits every box
        steps += 1
        assert steps <= len(a)
        if a["entry"][k] >= LEAF:
            seen.append(int(a["entry"][k] - LEAF))
            k = int(a["exit"][k])
        else:
            k = int(a["entry"][k])
    assert sorted(seen) == list(range(n_tris)), "every triangle exactly once"
    tlo, thi = prims[:n_tris].min(axis=1), prims[:n_tris].max(axis=1)
    for k in np.flatnonzero(~leaf):
        assert a["entry"][k] == k + 1 and k + 1 < a["exit"][k] <= len(a)
        shapes = (a["entry"][k + 1:a["exit"][k]][leaf[k + 1:a["exit"][k]]] - LEAF).astype(np.int64)
        assert np.array_equal(a["min"][k], tlo[shapes].min(axis=0)) and np.array_equal(a["max"][k], thi[shapes].max(axis=0)), k
    api = F.api()
    nodes = (F.HkNode * len(a)).from_buffer_copy(a.tobytes())
    out = (F.HkNode * len(a))()
    for octant in range(8):
        assert api.raw("bvh_rethread")(nodes, len(a), octant, out) == F.HK_OK, octant


def test_mixed_builder_builds_only_the_deferred_meshes():
    names = ("soup_3", "soup_1023", "strip", "half_split", "soup_1")
    deferred = (False, True, True, False, True)

    def build(twin):
        b = SceneBuilder()
        mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        ids = []
        for name, late in zip(names, deferred):
            p, idx, topology = MESHES[name]
            n, uv = flat(p)
            ids.append(b.add_mesh(p, n, uv, idx, topology, build_tree=twin or not late))
            if twin and late:
                b.rebuild_mesh_tree(ids[-1])
        for m in ids[:-1]:   # (the last mesh has no instance yet)
            b.add_instance(m, mat, IDENTITY)
        return b, ids

    d, ids = build(False)
    assert d.pending_mesh_trees() == 3
    before = node_array(d.finish().asset_nodes)
    d.build_pending_mesh_trees()
    assert d.pending_mesh_trees() == 0
    after = node_array(d.scene().asset_nodes)
    for m, late in zip(ids, deferred):
        i = d.mesh_index(m)
        same = after[i.node_offset:i.node_offset + i.node_count].tobytes() == before[i.node_offset:i.node_offset + i.node_count].tobytes()
        assert same == (not late or i.node_count == 1), (m, late)
    t, _ = build(True)
    assert after.tobytes() == bytes(t.finish().asset_nodes)
    # one more deferred mesh after the completion: only that one is pending, and its completion leaves the others' bytes alone
    p, idx, topology = MESHES["soup_1025"]
    n, uv = flat(p)
    d.add_mesh(p, n, uv, idx, topology, build_tree=False)
    assert d.pending_mesh_trees() == 1
    grown = node_array(d.finish().asset_nodes)
    assert grown[:len(after)].tobytes() == after.tobytes()
    d.build_pending_mesh_trees()
    assert node_array(d.scene().asset_nodes)[:len(after)].tobytes() == after.tobytes()
    # the twin's call on a pending mesh is its completion too
    e, eids = build(False)
    for m, late in zip(eids, deferred):
        if late:
            e.rebuild_mesh_tree(m)
    assert e.pending_mesh_trees() == 0
    assert bytes(e.finish().asset_nodes) == after.tobytes()


def test_oracle_renders_the_completed_builder_like_the_add_mesh_builder():
    import bevy_hikari_amd as hk
    from bevy_hikari_amd.scenes import synthetic_camera
    from oracle_lib import oracle_plugin

    def scene(late):
        b = SceneBuilder()
        mat = b.add_material(S.standard_material((0.7, 0.6, 0.5, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
        for k, name in enumerate(("soup_1023", "soup_3", "soup_2")):
            p, idx, topology = MESHES[name]
            n, uv = flat(p)
            m = b.add_mesh(p * np.float32(1.5), n, uv, idx, topology, build_tree=not late)
            b.add_instance(m, glow if k == 1 else mat, S._trs((0.0, 1.0, 0.0), (0.0, 0.3 * k, 0.0), (1.0, 1.0, 1.0)))
        out = b.finish()
        if late:
            b.build_pending_mesh_trees()
            out = b.scene()
        return out

    a, b = oracle_plugin(), oracle_plugin()
    a.set_scene(scene(True))
    b.set_scene(scene(False))
    cam, s = synthetic_camera(40, 28), hk.HikariSettings(indirect_bounces=1, upscale=hk.Upscale.SMAA_TU_1_0)
    for n in (1, 2):
        for p in (a, b):
            p.render(cam, s, frame_number=n)
        x, y = a.output(s), b.output(s)
        assert np.isfinite(y).all() and y.max() > 0.0
        assert x.tobytes() == y.tobytes(), f"frame {n}"


# ---------------------------------------------------------------------------------------------------------------- ABI
NEW = ("hk_scene_builder_add_mesh_deferred", "hk_scene_builder_pending_mesh_trees", "hk_scene_builder_build_pending_mesh_trees", "hk_load_scene", "hk_multi_load_scene")


def test_new_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "hikari_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "hikari-hip-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in F.DECLARED_SYMBOLS, name
        assert "pub fn " + name + "(" in rust, name
        assert F.api().raw(name[3:]) is not None
    assert "hk_debug_last_load(" in open(os.path.join(ROOT, "include", "hikari_hip_debug.h")).read()
    assert "hk_debug_last_load" in F.DECLARED_DEBUG_SYMBOLS
    assert F.api().abi_version() == 8   # (additive)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_argument_errors_without_a_device():
    api = F.api()
    n = F.u32(7)
    assert api.raw("scene_builder_pending_mesh_trees")(None, C.byref(n)) == F.HK_E_INVALID
    assert api.raw("scene_builder_build_pending_mesh_trees")(None) == F.HK_E_INVALID
    d, _ = builder_with("soup_3", "deferred")
    assert api.raw("scene_builder_pending_mesh_trees")(d.h, None) == F.HK_E_INVALID
    assert api.raw("load_scene")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("multi_load_scene")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    # the deferred form validates like add_mesh
    p, idx, _ = MESHES["soup_3"]
    nrm, uv = flat(p)
    fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
    bad = np.array([0, 1, 99], np.uint32)
    out = F.u32()
    for fn in ("scene_builder_add_mesh", "scene_builder_add_mesh_deferred"):
        assert api.raw(fn)(d.h, fp(p), fp(nrm), fp(uv), len(p), bad.ctypes.data_as(C.POINTER(F.u32)), 3, F.TOPOLOGY_TRIANGLE_LIST, C.byref(out)) == F.HK_E_INVALID
        assert api.raw(fn)(d.h, fp(p), None, fp(uv), len(p), None, 0, F.TOPOLOGY_TRIANGLE_LIST, C.byref(out)) == F.HK_E_INVALID
        assert api.raw(fn)(d.h, fp(p), fp(nrm), fp(uv), len(p), None, 0, 7, C.byref(out)) == F.HK_E_UNSUPPORTED
    assert d.pending_mesh_trees() == 1
