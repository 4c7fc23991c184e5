"""The host twin of the device's mesh-tree rebuild (hk_scene_builder_rebuild_mesh_tree): after a deformation it must give the tree a fresh
hk_scene_builder_add_mesh builds over the new positions - link for link, box for box - in the canonical form a refit leaves alone.  No
GPU needed."""
import ctypes as C

import numpy as np
import pytest

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder

NODE = np.dtype([("min", "<f4", 3), ("entry", "<u4"), ("max", "<f4", 3), ("exit", "<u4")])
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)


def node_array(nodes):
    return np.frombuffer(bytes(nodes), dtype=NODE).copy()


def flat(p):
    return np.tile(np.array([0, 1, 0], np.float32), (len(p), 1)), np.zeros((len(p), 2), np.float32)


def half_split_mesh(k=37, step=0.125):
    """k triangles whose boxes all have the centre (0, 0, 0) exactly: box k = [-s_k, s_k]^3.  The centre bounds have no extent, so
    BVH::build cuts the index list in half at every node."""
    s = (0.25 + step * np.arange(k)).astype(np.float32)
    p = np.stack([np.stack([-s, -s, -s], 1), np.stack([s, s, s], 1), np.stack([s, -s, np.zeros_like(s)], 1)], 1).reshape(-1, 3)
    return p.astype(np.float32), np.arange(3 * k, dtype=np.uint32)


def fixtures():
    """name -> (rest positions, deformed positions, indices)"""
    out = {}
    p, _, _, idx = S.cloth_grid(71, 71, size=2.0)   # 10 082 triangles
    out["folded_cloth"] = (p, S.folded_cloth(p)[0], idx)
    sp, _, _, sidx = S._sphere(12, 16)
    out["pulsing_sphere"] = (sp, S.pulsing_sphere(sp, 2), sidx)
    rng = np.random.default_rng(3)
    for k in (1, 2, 3):
        q = rng.uniform(-1, 1, (3 * k, 3)).astype(np.float32)
        out[f"{k}_triangles"] = (q, (q * np.float32(1.5) + np.float32(0.25)).astype(np.float32), np.arange(3 * k, dtype=np.uint32))
    hp, hidx = half_split_mesh()
    out["half_split"] = ((hp * np.float32(1.25) + np.float32(0.5)).astype(np.float32), hp, hidx)
    dp, _, _, didx = S.cloth_grid(6, 5, size=1.0)
    tri = didx.reshape(-1, 3)
    out["duplicated"] = (dp, S.waving_cloth(dp, 3, amplitude=0.4)[0], np.concatenate([tri, tri[::2], tri]).reshape(-1).astype(np.uint32))
    return out


FIXTURES = fixtures()


def builder_with(rest, idx, extra=True):
    """a builder holding [a bystander cloth,] the mesh under test [and a bystander sphere], one instance each"""
    b = SceneBuilder()
    mat = b.add_material(F.HkMaterial())
    ids = []
    if extra:
        p, n, uv, i = S.cloth_grid(5, 4)
        ids.append(b.add_mesh(p, n, uv, i))
    n, uv = flat(rest)
    mesh = b.add_mesh(rest, n, uv, idx)
    ids.append(mesh)
    if extra:
        p, n, uv, i = S._sphere(5, 6)
        ids.append(b.add_mesh(p, n, uv, i))
    for m in ids:
        b.add_instance(m, mat, IDENTITY)
    return b, mesh


def mesh_nodes(scene, b, mesh):
    i = b.mesh_index(mesh)
    return node_array(scene.asset_nodes)[i.node_offset:i.node_offset + i.node_count]


def fresh_nodes(positions, idx):
    b, mesh = builder_with(positions, idx, extra=False)
    return mesh_nodes(b.finish(), b, mesh)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_rebuild_after_a_deformation_equals_a_fresh_add_mesh(name):
    rest, new, idx = FIXTURES[name]
    b, mesh = builder_with(rest, idx)
    before = node_array(b.finish().asset_nodes)
    index = b.mesh_index(mesh)
    lo, hi = index.node_offset, index.node_offset + index.node_count
    b.set_mesh_vertices(mesh, new)
    b.rebuild_mesh_tree(mesh)
    scene = b.finish()
    got, want = mesh_nodes(scene, b, mesh), fresh_nodes(new, idx)
    assert np.array_equal(got["entry"], want["entry"]) and np.array_equal(got["exit"], want["exit"]), "links differ from a fresh build's, node for node"
    assert np.array_equal(got["min"], want["min"]) and np.array_equal(got["max"], want["max"]), "boxes differ from a fresh build's"
    # the other meshes' nodes: the same bytes as before
    after = node_array(scene.asset_nodes)
    assert after[:lo].tobytes() == before[:lo].tobytes() and after[hi:].tobytes() == before[hi:].tobytes()
    # the boxes are canonical already: a refit over the same positions changes no byte
    b.set_mesh_vertices(mesh, new)
    assert mesh_nodes(b.finish(), b, mesh).tobytes() == got.tobytes()
    # every octant's re-threading takes the tree
    api = F.api()
    nodes = (F.HkNode * len(got)).from_buffer_copy(got.tobytes())
    out = (F.HkNode * len(got))()
    for octant in range(8):
        assert api.raw("bvh_rethread")(nodes, len(got), octant, out) == F.HK_OK, octant


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_rebuild_without_a_deformation_keeps_the_links(name):
    rest, _, idx = FIXTURES[name]
    b, mesh = builder_with(rest, idx)
    before = mesh_nodes(b.finish(), b, mesh)
    b.rebuild_mesh_tree(mesh)
    after = mesh_nodes(b.finish(), b, mesh)
    assert np.array_equal(after["entry"], before["entry"]) and np.array_equal(after["exit"], before["exit"])
    assert np.array_equal(after["min"], before["min"]) and np.array_equal(after["max"], before["max"])


def test_the_half_split_fixture_takes_the_half_split_path():
    """every navigator of the half-split mesh covers floor(n / 2) leaves first: the tree of halved index lists"""
    _, new, idx = FIXTURES["half_split"]
    a = fresh_nodes(new, idx)
    k = len(idx) // 3

    def walk(begin, end, count):   # the subtree [begin, end) over `count` shapes
        if count == 1:
            return
        left = count // 2
        assert a["exit"][begin] == begin + 1 + 3 * left - 2, (begin, count)
        walk(begin + 1, a["exit"][begin], left)
        second = a["exit"][begin]
        walk(second + 1, end, count - left)

    walk(0, len(a), k)


def test_unknown_mesh_id_changes_nothing():
    rest, new, idx = FIXTURES["pulsing_sphere"]
    b, mesh = builder_with(rest, idx)
    b.finish()
    b.set_mesh_vertices(mesh, new)
    names = ("vertices", "primitives", "asset_nodes", "instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table")
    before = b.finish()
    snap = {n: bytes(getattr(before, n)) for n in names}
    api = F.api()
    assert api.raw("scene_builder_rebuild_mesh_tree")(b.h, 3) == F.HK_E_INVALID
    assert api.raw("scene_builder_rebuild_mesh_tree")(b.h, 0xFFFFFFFF) == F.HK_E_INVALID
    assert api.raw("scene_builder_rebuild_mesh_tree")(None, mesh) == F.HK_E_INVALID
    after = b.finish()
    for n in names:
        assert bytes(getattr(after, n)) == snap[n], n


def test_device_entry_points_refuse_null_arguments():
    api = F.api()
    mi = F.HkMeshIndex()
    assert api.raw("rebuild_mesh_tree")(None, C.byref(mi), F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("multi_rebuild_mesh_tree")(None, C.byref(mi), F.TREE_SAH) == F.HK_E_INVALID
