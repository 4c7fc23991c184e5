"""The host side of hk_remove_meshes: hk_scene_builder_remove_mesh leaves, after the next finish, the builder that never had the mesh -
getter for getter and byte for byte - and returns the mesh's extent in the coordinates of the last finish, which is what the context's
compaction takes; hk_rebase_mesh_index is held against a numpy restatement of its rule."""
import ctypes as C
import re

import numpy as np
import pytest

from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from conftest import ROOT
from test_add_meshes import BUFFERS, record, soup
from test_mesh_rebuild import IDENTITY, flat

# (triangles, deferred, instances): odd sizes, a one-triangle mesh, meshes without an instance, deferred ones
SPECS = [(30, False, 1), (1, False, 0), (257, True, 2), (2, False, 1), (64, True, 0), (7, False, 1)]


def build(specs):
    """(builder, mesh ids): every mesh of `specs`, `instances` instances each (one emits, so that the emissive arrays are not empty)"""
    b = SceneBuilder()
    b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    ids = []
    for triangles, deferred, instances in specs:
        p, i = soup(triangles, 40 + triangles)
        n, uv = flat(p)
        m = b.add_mesh(p, n, uv, i, build_tree=not deferred)
        ids.append(m)
        for k in range(instances):
            b.add_instance(m, k % 2, pose(triangles, k))
    return b, ids


def pose(triangles, k):
    """(by the mesh's size, not its id: the twin's ids differ)"""
    return S._trs((0.01 * triangles, 0.2 * k, 0.0), (0.0, 0.003 * triangles, 0.0), (1.0, 1.0, 1.0))


def extent(e):
    return (e.vertex, e.n_vertices, e.primitive, e.n_primitives, e.node_offset, e.node_count)


def getters(b):
    s = b.scene()
    out = {n: bytes(getattr(s, n)) for n in BUFFERS}
    prev = (C.POINTER(F.f32))()
    n = F.u32()
    b.api.call("scene_builder_previous_transforms", b.h, C.byref(prev), C.byref(n))
    out["previous_transforms"] = bytes(C.cast(prev, C.POINTER(F.f32 * (16 * max(1, n.value)))).contents)[:64 * n.value]
    return out


def assert_equal_to_twin(b, twin, n_meshes, what):
    got, want = getters(b), getters(twin)
    for name in want:
        assert got[name] == want[name], f"{what}: {name} differ from the builder that never had the meshes"
    for m in range(n_meshes):
        assert record(b.mesh_index(m)) == record(twin.mesh_index(m)), f"{what}: the record of mesh {m}"
        assert extent(b.mesh_extent(m)) == extent(twin.mesh_extent(m)), f"{what}: the extent of mesh {m}"
    assert b.pending_mesh_trees() == twin.pending_mesh_trees()
    assert b.api.raw("scene_builder_mesh_index")(b.h, n_meshes, C.byref(F.HkMeshIndex())) == F.HK_E_INVALID


def strip_instances(specs, gone):
    """the specs with the instances of the meshes `gone` taken away (a mesh leaves only once nothing names it)"""
    return [(t, d, 0 if k in gone else n) for k, (t, d, n) in enumerate(specs)]


@pytest.mark.parametrize("gone", [[0], [5], [2, 3], [1, 3, 5], [0, 1, 2, 3, 4]], ids=["first", "last", "neighbours", "every-second", "all-but-one"])
@pytest.mark.parametrize("finished", [True, False], ids=["finished", "unfinished"])
def test_a_removed_mesh_leaves_the_builder_that_never_had_it(gone, finished):
    specs = strip_instances(SPECS, gone)
    if gone == [0, 1, 2, 3, 4]:
        specs[5] = (7, False, 2)   # (the survivor carries every instance: an emitter among them)
    b, ids = build(specs)
    twin, _ = build([s for k, s in enumerate(specs) if k not in gone])
    if finished:
        b.finish()
        last = {m: (record(b.mesh_index(m)), len(soup(specs[m][0], 40 + specs[m][0])[0])) for m in ids}
    extents = []
    for m in sorted(gone, reverse=True):   # (back to front: the ids in front of a removed mesh stay)
        extents.append((m, extent(b.remove_mesh(m))))
    if finished:   # the extent is the record and the vertex count of the last finish - every removal in the same coordinates
        for m, e in extents:
            (vertex, primitive, node_offset, node_count), n_vertices = last[m]
            assert e == (vertex, n_vertices, primitive, (node_count + 2) // 3, node_offset, node_count), m
    else:
        assert all(e[5] == 0 for _, e in extents), "a mesh no finish has seen lies in no array"
    assert b.api.raw("scene_builder_vertices")(b.h, C.byref(C.POINTER(F.HkVertex)()), C.byref(F.u32())) == F.HK_E_NOT_READY, "the removal un-finishes the builder"
    b.finish()
    twin.finish()
    assert_equal_to_twin(b, twin, len(SPECS) - len(gone), f"without {gone}")


def test_ids_and_instance_declarations_shift_down():
    b, ids = build(strip_instances(SPECS, [1]))
    b.finish()
    before = [record(b.mesh_index(m)) for m in ids]
    b.remove_mesh(1)
    scene = b.finish()
    after = [record(b.mesh_index(m)) for m in range(len(ids) - 1)]
    assert after[0] == before[0]
    for m in range(1, len(after)):   # mesh m was mesh m + 1: the same counts, the offsets minus the removed mesh's
        assert after[m][3] == before[m + 1][3]
        assert after[m][2] == before[m + 1][2] - before[1][3] and after[m][1] == before[m + 1][1] - (before[1][3] + 2) // 3
    inst = np.frombuffer(bytes(scene.instances), np.uint8).reshape(-1, C.sizeof(F.HkInstance))
    meshes = [record(F.HkInstance.from_buffer_copy(row.tobytes()).mesh) for row in inst]
    want = [after[m - 1 if m > 1 else m] for m, (_, _, n) in enumerate(SPECS) if m != 1 for _ in range(n)]
    assert meshes == want


def test_a_mesh_added_after_the_finish_has_no_extent_and_a_removed_deferred_mesh_takes_its_mark():
    b, ids = build(strip_instances(SPECS, [2, 4]))
    b.finish()
    assert b.pending_mesh_trees() == 2
    p, i = soup(11, 9)
    n, uv = flat(p)
    late = b.add_mesh(p, n, uv, i, build_tree=False)
    assert b.pending_mesh_trees() == 3
    assert extent(b.mesh_extent(late)) == (0, 0, 0, 0, 0, 0)
    assert extent(b.remove_mesh(late)) == (0, 0, 0, 0, 0, 0) and b.pending_mesh_trees() == 2
    e4, e2 = extent(b.mesh_extent(4)), extent(b.mesh_extent(2))
    assert extent(b.remove_mesh(4)) == e4 and b.pending_mesh_trees() == 1
    assert extent(b.mesh_extent(2)) == e2, "the extents stay in the coordinates of the last finish until the next one"
    assert extent(b.remove_mesh(2)) == e2 and b.pending_mesh_trees() == 0
    twin, _ = build([s for k, s in enumerate(strip_instances(SPECS, [2, 4])) if k not in (2, 4)])
    b.finish()
    twin.finish()
    assert_equal_to_twin(b, twin, 4, "without the deferred meshes")


def test_refusals_leave_a_finished_builder_finished_and_every_byte_unchanged():
    b, ids = build(SPECS)
    b.finish()
    before = getters(b)
    records = [record(b.mesh_index(m)) for m in ids]
    api = b.api
    out = F.HkMeshExtent()
    assert api.raw("scene_builder_remove_mesh")(b.h, 0, C.byref(out)) == F.HK_E_INVALID and "still names" in api.last_error()   # in use
    assert api.raw("scene_builder_remove_mesh")(b.h, len(ids), None) == F.HK_E_INVALID   # unknown id
    assert api.raw("scene_builder_remove_mesh")(None, 1, None) == F.HK_E_INVALID
    assert api.raw("scene_builder_mesh_extent")(b.h, len(ids), C.byref(out)) == F.HK_E_INVALID
    assert api.raw("scene_builder_mesh_extent")(b.h, 0, None) == F.HK_E_INVALID
    assert getters(b) == before   # (the getters of an unfinished builder would raise)
    assert [record(b.mesh_index(m)) for m in ids] == records and b.pending_mesh_trees() == 2
    # with NULL for the extent the removal itself is accepted
    assert api.raw("scene_builder_remove_mesh")(b.h, 1, None) == F.HK_OK


def test_remove_then_add_equals_the_builder_given_that_mesh_set_from_the_start():
    specs = strip_instances(SPECS, [1, 4])
    b, _ = build(specs)
    b.finish()
    b.remove_mesh(4)
    b.remove_mesh(1)
    extra = [(90, True, 1), (3, False, 1)]
    for triangles, deferred, instances in extra:
        p, i = soup(triangles, 40 + triangles)
        n, uv = flat(p)
        m = b.add_mesh(p, n, uv, i, build_tree=not deferred)
        for k in range(instances):
            b.add_instance(m, k % 2, pose(triangles, k))
    b.finish()
    # the twin's instances in the order the edited builder declared them: every instance of the old meshes first
    twin, _ = build([s for k, s in enumerate(specs) if k not in (1, 4)] + [(t, d, 0) for t, d, _ in extra])
    for m, (triangles, _, _) in zip((4, 5), extra):
        twin.add_instance(m, 0, pose(triangles, 0))
    twin.finish()
    assert_equal_to_twin(b, twin, 6, "remove, add, finish")


# ---------------------------------------------------------------------------------------------------------------- hk_rebase_mesh_index
def rebase_numpy(extents, index):
    """each of vertex, primitive, node_offset minus the removed elements in front of it"""
    out = list(index)
    e = np.array([x for x in extents if x[5] != 0], np.int64).reshape(-1, 6)
    for field, (begin, count) in enumerate(((0, 1), (2, 3), (4, 5))):
        gone = np.clip(index[field] - e[:, begin], 0, e[:, count]).sum() if len(e) else 0
        out[field] = index[field] - int(gone)
    return tuple(out)


def call_rebase(extents, index):
    arr = (F.HkMeshExtent * max(1, len(extents)))(*[F.HkMeshExtent(*x) for x in extents])
    out = F.HkMeshIndex()
    F.api().call("rebase_mesh_index", arr, len(extents), C.byref(F.HkMeshIndex(*index)), C.byref(out))
    return record(out)


def test_rebase_mesh_index_against_numpy_over_random_extent_sets():
    rng = np.random.default_rng(5)
    assert call_rebase([], (7, 5, 13, 13)) == (7, 5, 13, 13)
    api = F.api()
    assert api.raw("rebase_mesh_index")(None, 1, C.byref(F.HkMeshIndex()), C.byref(F.HkMeshIndex())) == F.HK_E_INVALID
    assert api.raw("rebase_mesh_index")(None, 0, None, C.byref(F.HkMeshIndex())) == F.HK_E_INVALID
    assert api.raw("rebase_mesh_index")(None, 0, C.byref(F.HkMeshIndex(1, 2, 3, 4)), None) == F.HK_E_INVALID
    for trial in range(200):
        n = int(rng.integers(0, 9))
        # disjoint extents in ascending order in all three ranges, some of them of meshes no finish had seen (node_count 0)
        extents, at = [], [0, 0, 0]
        for _ in range(n):
            tris = int(rng.integers(1, 50))
            counts = (int(rng.integers(1, 150)), tris, 3 * tris - 2)
            start = [a + int(rng.integers(0, 40)) for a in at]
            seen = rng.random() > 0.15
            extents.append((start[0], counts[0], start[1], counts[1], start[2], counts[2] if seen else 0))
            at = [s + c for s, c in zip(start, counts)]
        order = rng.permutation(n)
        shuffled = [extents[k] for k in order]
        # records in front of every extent, behind all of them, between two, and inside one (the extent lies around the record)
        picks = [(0, 0, 0)] + [tuple(a + int(rng.integers(0, 30)) for a in at)]
        for e in extents:
            picks.append((e[0] + e[1], e[2] + e[3], e[4] + (e[5] or 3 * e[3] - 2)))
            picks.append((e[0] + e[1] // 2, e[2] + e[3] // 2, e[4] + e[5] // 2))
        for vertex, primitive, node_offset in picks:
            index = (vertex, primitive, node_offset, 3 * int(rng.integers(1, 9)) - 2)
            assert call_rebase(shuffled, index) == rebase_numpy(shuffled, index), (trial, shuffled, index)


def test_rebase_equals_the_records_of_the_next_finish():
    specs = strip_instances(SPECS, [1, 2, 4])
    b, ids = build(specs)
    b.finish()
    before = {m: record(b.mesh_index(m)) for m in ids}
    removed = [extent(b.remove_mesh(m)) for m in (4, 2, 1)]
    b.finish()
    for new, old in enumerate((0, 3, 5)):
        assert call_rebase(removed, before[old]) == record(b.mesh_index(new))


def test_the_new_symbols_are_declared_and_the_abi_number_stays():
    header = open(f"{ROOT}/include/hikari_hip.h").read()
    debug = open(f"{ROOT}/include/hikari_hip_debug.h").read()
    assert re.search(r"#define\s+HK_ABI_VERSION\s+8\b", header) and F.api().abi_version() == 8
    assert C.sizeof(F.HkMeshExtent) == 24
    assert re.search(r"int hk_remove_meshes\(hk_ctx\* ctx, const HkMeshExtent\* removed, uint32_t n\);", header)
    assert re.search(r"int hk_multi_remove_meshes\(hk_multi\* m, const HkMeshExtent\* removed, uint32_t n\);", header)
    assert re.search(r"int hk_scene_builder_remove_mesh\(hk_scene_builder\* b, uint32_t mesh_id, HkMeshExtent\* removed\);", header)
    assert re.search(r"int hk_debug_last_remove\(hk_ctx\* ctx, uint64_t out\[6\]\);", debug)
    api = F.api()
    assert api.raw("remove_meshes")(None, None, 0) == F.HK_E_INVALID
    assert api.raw("multi_remove_meshes")(None, None, 0) == F.HK_E_INVALID
    assert api.raw("debug_last_remove")(None, None) == F.HK_E_INVALID


def test_no_parameter_or_field_of_the_rust_binding_is_named_by_a_rust_keyword():
    """a C parameter called `in` would stop the whole crate from compiling: the generator refuses such names, and the committed file has none"""
    import sys

    sys.path.insert(0, f"{ROOT}/tools")
    import gen_rust_ffi

    text = open(f"{ROOT}/rust/hikari-hip-sys/src/lib.rs").read()
    names = re.findall(r"[(,]\s*(\w+): ", text) + re.findall(r"pub (\w+): ", text)
    assert len(names) > 300 and "index" in names
    assert [n for n in names if n in gen_rust_ffi.RUST_KEYWORDS] == []
    api = gen_rust_ffi.parse_header()
    api["functions"].append(("hk_bad", "int", [("in", "uint32_t", False, 0, False)]))
    with pytest.raises(AssertionError, match="Rust keyword"):
        gen_rust_ffi.emit(api)
