"""The host side of hk_add_meshes: a builder that is finished again after meshes were added appends them to its concatenated arrays -
every HkMeshIndex and the old prefix of the three arrays stay, and the result is the builder given all meshes at once."""
import ctypes as C
import re

import numpy as np

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from conftest import ROOT
from test_mesh_rebuild import IDENTITY, flat

ARRAYS = ("vertices", "primitives", "asset_nodes")
BUFFERS = ARRAYS + ("materials", "instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table")


def soup(k, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (k, 1, 3))
    return (c + rng.uniform(-0.05, 0.05, (k, 3, 3))).reshape(-1, 3).astype(np.float32), np.arange(3 * k, dtype=np.uint32)


def add_meshes(b, specs):
    ids = []
    for k, (triangles, deferred) in enumerate(specs):
        p, i = soup(triangles, 40 + triangles)
        n, uv = flat(p)
        ids.append(b.add_mesh(p, n, uv, i, build_tree=not deferred))
    return ids


def record(index):
    return (index.vertex, index.primitive, index.node_offset, index.node_count)


FIRST = [(30, False), (1, False), (257, False)]
LATER = [(2, True), (64, False), (500, True)]


def test_a_finish_after_added_meshes_keeps_the_old_prefix_and_equals_one_finish_of_everything():
    b, whole = SceneBuilder(), SceneBuilder()
    for q in (b, whole):
        q.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    ids = add_meshes(b, FIRST)
    for m in ids:
        b.add_instance(m, 0, IDENTITY)
    first = b.finish()
    old = {n: bytes(getattr(first, n)) for n in ARRAYS}
    old_records = [record(b.mesh_index(m)) for m in ids]
    later = add_meshes(b, LATER)
    grown = b.finish()
    assert [record(b.mesh_index(m)) for m in ids] == old_records
    for n in ARRAYS:
        assert bytes(getattr(grown, n))[:len(old[n])] == old[n], f"the old prefix of {n} changed"
        assert len(bytes(getattr(grown, n))) > len(old[n])
    at = old_records[-1]
    for m in later:   # the new ranges lie behind the old ones, in id order
        r = record(b.mesh_index(m))
        assert r[1] == at[1] + (at[3] + 2) // 3 and r[2] == at[2] + at[3] and r[0] > at[0]
        at = r
    # ... and a change to an EXISTING mesh after that is still taken up by the next finish
    for m in add_meshes(whole, FIRST + LATER)[:len(FIRST)]:
        whole.add_instance(m, 0, IDENTITY)
    everything = whole.finish()
    for n in BUFFERS:
        assert bytes(getattr(grown, n)) == bytes(getattr(everything, n)), f"{n} differ from the builder given all meshes at once"
    assert b.pending_mesh_trees() == whole.pending_mesh_trees() == 2
    for q in (b, whole):
        q.rebuild_mesh_tree(1)
        q.rebuild_mesh_tree(3)
    g, e = b.finish(), whole.finish()
    for n in BUFFERS:
        assert bytes(getattr(g, n)) == bytes(getattr(e, n)), f"{n} differ after a change to existing meshes"
    assert b.pending_mesh_trees() == 1


def test_pending_trees_completed_after_a_mesh_was_added_reach_the_concatenated_array():
    """add_mesh_deferred(A), finish, add_mesh(B), build_pending_mesh_trees, finish: A's tree is completed while the concatenated arrays are
    out of date - the next finish must not keep A's stand-in in the prefix it appends to."""
    (pa, ia), (pb, ib) = soup(90, 3), soup(40, 4)

    def put(q, positions, idx, deferred):
        n, uv = flat(positions)
        return q.add_mesh(positions, n, uv, idx, build_tree=not deferred)

    b, whole = SceneBuilder(), SceneBuilder()
    for q in (b, whole):
        q.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    a = put(b, pa, ia, True)
    b.add_instance(a, 0, IDENTITY)
    standin = bytes(b.finish().asset_nodes)
    put(b, pb, ib, False)
    b.build_pending_mesh_trees()
    got = b.finish()
    whole.add_instance(put(whole, pa, ia, True), 0, IDENTITY)
    put(whole, pb, ib, False)
    whole.build_pending_mesh_trees()
    want = whole.finish()
    assert b.pending_mesh_trees() == whole.pending_mesh_trees() == 0
    assert bytes(got.asset_nodes)[:len(standin)] != standin, "the stand-in tree is still in the concatenated array"
    for n in BUFFERS:
        assert bytes(getattr(got, n)) == bytes(getattr(want, n)), f"{n} differ from the builder given everything at once"
    # ... and completed while the arrays ARE up to date (finish, then build): patched in place, and a later append keeps it
    c = SceneBuilder()
    c.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    c.add_instance(put(c, pa, ia, True), 0, IDENTITY)
    c.finish()
    c.build_pending_mesh_trees()
    put(c, pb, ib, False)
    again = c.finish()
    for n in BUFFERS:
        assert bytes(getattr(again, n)) == bytes(getattr(want, n)), f"{n} differ after build, add, finish"


def test_the_new_symbols_are_declared_and_the_abi_number_stays():
    header = open(f"{ROOT}/include/hikari_hip.h").read()
    debug = open(f"{ROOT}/include/hikari_hip_debug.h").read()
    assert re.search(r"#define\s+HK_ABI_VERSION\s+8\b", header) and F.api().abi_version() == 8
    assert re.search(r"int hk_add_meshes\(hk_ctx\* ctx, hk_scene_builder\* b, uint32_t tree_mode\);", header)
    assert re.search(r"int hk_multi_add_meshes\(hk_multi\* m, hk_scene_builder\* b, uint32_t tree_mode\);", header)
    assert re.search(r"int hk_debug_last_add\(hk_ctx\* ctx, uint32_t out\[5\]\);", debug)
    api = F.api()
    for name in ("add_meshes", "multi_add_meshes", "debug_last_add", "debug_last_add_times"):
        fn = api.raw(name)
        assert fn is not None and fn.restype is C.c_int, name
    assert len(api.raw("add_meshes").argtypes) == 3 and len(api.raw("debug_last_add").argtypes) == 2


def test_add_meshes_refuses_null_arguments_without_a_device():
    api = F.api()
    b = SceneBuilder()
    assert api.raw("add_meshes")(None, b.h, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("multi_add_meshes")(None, b.h, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("debug_last_add")(None, None) == F.HK_E_INVALID
