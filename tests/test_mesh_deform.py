"""Mesh deformation, host side: the builder's mirror of a device refit (hk_scene_builder_set_mesh_vertices) and the argument checks of
the deformation entry points (hikari_hip.h hk_update_mesh_vertices / hk_set_mesh_skin / hk_skin_mesh).  No GPU needed."""
import ctypes as C

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder

LEAF = 0x80000000


def leaf_box(prims, shape):
    v = np.array([list(prims[shape].vertices[k].position) for k in range(3)], dtype=np.float32)
    return v.min(axis=0), v.max(axis=0)


def check_union(nodes, prims):
    """every navigator's box = the numpy union of the triangle boxes of the leaves in its subtree (i, exit)"""
    entry = np.array([n.entry_index for n in nodes], dtype=np.int64)
    for i, n in enumerate(nodes):
        if entry[i] >= LEAF:
            assert list(n.min) == [float("inf")] * 3 and list(n.max) == [float("-inf")] * 3, "a leaf keeps the empty box bvh 0.7.1 stores"
            continue
        boxes = [leaf_box(prims, int(entry[j] - LEAF)) for j in range(i + 1, n.exit_index) if entry[j] >= LEAF]
        mn = np.min([b[0] for b in boxes], axis=0)
        mx = np.max([b[1] for b in boxes], axis=0)
        assert np.array_equal(np.array(list(n.min), np.float32), mn) and np.array_equal(np.array(list(n.max), np.float32), mx), f"node {i}"


def mesh_slice(scene, index, arr):
    return arr[index.node_offset:index.node_offset + index.node_count]


def test_set_mesh_vertices_keeps_links_and_refits_every_box():
    b = SceneBuilder()
    p, n, uv, idx = S.cloth_grid(10, 7, size=2.0)
    mesh = b.add_mesh(p, n, uv, idx)
    mat = b.add_material(F.HkMaterial())
    b.add_instance(mesh, mat, np.eye(4, dtype=np.float32).reshape(-1))
    before = b.finish()
    index = b.mesh_index(mesh)
    assert (index.vertex, index.primitive, index.node_offset, index.node_count) == (0, 0, 0, 3 * 140 - 2)
    for frame in (1, 5):
        q, qn = S.waving_cloth(p, frame, amplitude=0.3)
        b.set_mesh_vertices(mesh, q, qn)
        after = b.finish()
        assert [(x.entry_index, x.exit_index) for x in after.asset_nodes] == [(x.entry_index, x.exit_index) for x in before.asset_nodes]
        prims = after.primitives
        for t in range(len(prims)):
            for k in range(3):
                v = prims[t].vertices[k]
                assert list(v.position) == q[v.index].tolist()
        check_union(after.asset_nodes, prims)
        verts = np.array([list(v.position) for v in after.vertices], np.float32)
        assert np.array_equal(verts, q) and np.array_equal(np.array([list(v.normal) for v in after.vertices], np.float32), qn)
        # the instance box follows the new mesh box (identity transform: the box itself)
        lo, hi = q.min(axis=0), q.max(axis=0)
        assert np.allclose(list(after.instances[0].min), lo) and np.allclose(list(after.instances[0].max), hi)
    # normals = NULL keeps them
    b.set_mesh_vertices(mesh, p)
    kept = b.finish()
    assert np.array_equal(np.array([list(v.normal) for v in kept.vertices], np.float32), qn)


def test_builder_mirror_argument_errors():
    api = F.api()
    b = SceneBuilder()
    p, n, uv, idx = S.cloth_grid(2, 2)
    mesh = b.add_mesh(p, n, uv, idx)
    out = F.HkMeshIndex()
    assert api.raw("scene_builder_mesh_index")(b.h, mesh, C.byref(out)) == F.HK_E_INVALID  # not finished since the mesh was added
    b.add_instance(mesh, b.add_material(F.HkMaterial()), np.eye(4, dtype=np.float32).reshape(-1))
    b.finish()
    assert api.raw("scene_builder_mesh_index")(b.h, mesh + 1, C.byref(out)) == F.HK_E_INVALID
    assert api.raw("scene_builder_mesh_index")(b.h, mesh, None) == F.HK_E_INVALID
    fp = p.ctypes.data_as(C.POINTER(F.f32))
    assert api.raw("scene_builder_set_mesh_vertices")(b.h, mesh + 1, fp, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_set_mesh_vertices")(b.h, mesh, None, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_set_mesh_vertices")(None, mesh, fp, None) == F.HK_E_INVALID


def test_device_entry_points_refuse_null_arguments():
    api = F.api()
    mi = F.HkMeshIndex()
    pos = np.zeros((4, 3), np.float32).ctypes.data_as(C.POINTER(F.f32))
    assert api.raw("update_mesh_vertices")(None, C.byref(mi), 4, pos, None) == F.HK_E_INVALID
    assert api.raw("skin_mesh")(None, C.byref(mi), pos, 1) == F.HK_E_INVALID
    assert api.raw("set_mesh_skin")(None, C.byref(mi), 4, pos, pos, None, pos) == F.HK_E_INVALID
    assert api.raw("multi_update_mesh_vertices")(None, C.byref(mi), 4, pos, None) == F.HK_E_INVALID


def test_skin_reference_is_the_identity_for_identity_joints():
    p, n, uv, idx, ji, jw = S.bending_cylinder()
    joints = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (3, 1))
    single = jw.sum(axis=1) == 1.0
    q, qn = S.skin_reference(p, n, ji, jw, joints)
    assert np.array_equal(q[single], p[single]) and np.array_equal(qn[single], n[single])
    assert (jw.sum(axis=1) != 1.0).any() and (jw[:, 1:] == 0).all(axis=1).any(), "the cylinder carries both kinds of weights"
