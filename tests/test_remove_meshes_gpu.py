"""hk_remove_meshes: meshes removed from a loaded scene, the mesh-level region compacted on the device.  A context that held meshes and
had them removed must hold, byte for byte, what a fresh context holds after hk_upload_scene of the twin builder that never had them -
nodes in every ordering, the geometry of every survivor, every buffer of the frames that follow.  The base scene lies beyond the LDS copy
(a 1 100-triangle soup); the meshes around it have 1, 2, 3, 7, 40, 300 and 1 025 triangles, odd vertex counts and - the mesh of 40 -
vertices no triangle names, so the runs shift the uv plane by 8 B and the rank plane by 4, 8 and 12 B modulo 16, and some runs are
shorter than one lane's 16 B.  Every case runs with the product's default traversal (8 orderings, wide records and ranks) and under the
suite's HK_CTX_EXACT_TRAVERSAL (1 ordering)."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder, make_rays
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from test_add_meshes_gpu import MODES, SUN, add, mesh_builds, place, plugin, view
from test_mesh_deform_gpu import SETTINGS
from test_mesh_rebuild_gpu import soup
from test_scene_load_gpu import nodes_equal, render_and_compare

pytestmark = pytest.mark.gpu

SIZES = [7, 1100, 1, 2, 3, 40, 300, 1025]   # mesh k has SIZES[k] triangles; mesh 1 keeps every scene beyond the LDS copy
ALL = list(range(len(SIZES)))
_DATA = {}


def mesh_data(k):
    """(positions, normals, uvs, indices) of mesh k: a soup with uvs that differ vertex by vertex; the mesh of 40 triangles carries three
    vertices no triangle names (123 vertices)"""
    if k not in _DATA:
        p, _, i = soup(SIZES[k], 700 + k)
        if SIZES[k] == 40:
            p = np.concatenate([p, p[:3] + np.float32(0.01)])
        rng = np.random.default_rng(900 + k)
        n = rng.normal(size=p.shape).astype(np.float32)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        _DATA[k] = (p, n.astype(np.float32), rng.uniform(0.0, 1.0, (len(p), 2)).astype(np.float32), i)
    return _DATA[k]


def build(keep=ALL, instanced=ALL):
    """(finished builder, material, {k: mesh id}): the meshes `keep` in order, one instance of each that is in `instanced`"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    ids = {k: b.add_mesh(*mesh_data(k)) for k in keep}
    for k in keep:
        if k in instanced:
            b.add_instance(ids[k], mat, place(k))
    b.finish()
    return b, mat, ids


def remove(target, d, ids, gone, instanced=None):
    """the meshes `gone` leave builder `d` and `target` (a plugin or a multi engine): their instances first (where they have any), then the
    meshes, back to front - every extent in the coordinates of the one finish in front of them - then the finish that gives the survivors
    their new records"""
    if instanced:
        order = [k for k in sorted(ids) if k in instanced]
        for k in sorted((k for k in gone if k in instanced), reverse=True):
            d.remove_instance(order.index(k))
        target.engine.update_instances_on_device(d, F.TREE_SAH)
    extents = [d.remove_mesh(ids[k]) for k in sorted(gone, reverse=True)]
    target.remove_meshes(extents)
    d.finish()
    return extents


def survivors_equal(gpu, twin, t, n_meshes, what):
    """nodes in every ordering, and the geometry of the meshes 0 .. n_meshes - 1 (each carried by an instance) under their new records"""
    nodes_equal(gpu, twin, what)
    for m in range(n_meshes):
        index = t.mesh_index(m)
        g, w = gpu.engine.read_mesh_geometry(index), twin.engine.read_mesh_geometry(index)
        for key in ("positions", "normals", "triangles", "box"):
            assert g[key].tobytes() == w[key].tobytes(), f"{what}: {key} of mesh {m} differ from the twin's"


GONE = {"first": [0], "last": [7], "neighbours": [3, 4], "every-second": [0, 2, 4, 6], "all-but-one": [0, 2, 3, 4, 5, 6, 7]}


# ---------------------------------------------------------------------------------------------------------------- 1. equal to the twin
@MODES
@pytest.mark.parametrize("which", list(GONE))
def test_removed_meshes_leave_the_twin_that_never_had_them(threaded, which):
    gone = GONE[which]
    left = [k for k in ALL if k not in gone]
    d, _, ids = build()
    t, _, _ = build(left, left)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    cam, lights, s = view()
    # a ray query lays the scene out and, in default mode, derives the wide records and ranks that the removal then moves (a frame would
    # leave instance ids of the larger instance set in the reservoirs' history, which the twin never had)
    rng = np.random.default_rng(4)
    origins = rng.uniform(-3.0, 3.0, (256, 3)).astype(np.float32)
    gpu.engine.cast_rays(make_rays(origins, rng.uniform(-1.0, 1.5, (256, 3)).astype(np.float32) - origins))
    twin.set_scene(t.scene())
    builds = mesh_builds(gpu)
    extents = remove(gpu, d, ids, gone, ALL)
    meshes, tris, launches, runs, path, moved = gpu.engine.last_remove()
    print(f"{which}: {meshes} meshes / {tris} triangles, {launches} launches, {runs} runs per plane, path {path}, {moved} bytes moved")
    assert (meshes, tris, path) == (len(gone), sum(SIZES[k] for k in gone), 0) and launches > 0 and moved > 0
    assert mesh_builds(gpu) == builds, "the removal laid the mesh level out again on the host"
    for new, k in enumerate(left):   # the records after the finish are the rebased ones
        assert bytes(d.mesh_index(new)) == bytes(t.mesh_index(new))
    survivors_equal(gpu, twin, t, len(left), which)
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), which)
    assert mesh_builds(gpu) == builds


# ---------------------------------------------------------------------------------------------------------------- 2. launches
@MODES
def test_launches_do_not_follow_the_number_of_meshes(threaded):
    def sixty(keep):
        b = SceneBuilder()
        mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
        b.add_instance(b.add_mesh(*mesh_data(1)), mat, place(1))
        ids = []
        for k in keep:
            p, _, i = soup((1, 2, 3, 5, 7)[k % 5], 300 + k)
            ids.append(add(b, "twin", p, i, deferred=False))
        b.finish()
        return b, ids

    results = {}
    for name, gone in (("one", [30]), ("alternating", list(range(0, 60, 2)))):
        d, ids = sixty(range(60))
        gpu = plugin(threaded)
        gpu.set_scene(d.scene())
        gpu.engine.read_mesh_nodes()
        builds = mesh_builds(gpu)
        gpu.remove_meshes([d.remove_mesh(ids[k]) for k in sorted(gone, reverse=True)])
        results[name] = gpu.engine.last_remove()
        assert results[name][0] == len(gone) and results[name][4] == 0 and mesh_builds(gpu) == builds, results
        t, _ = sixty([k for k in range(60) if k not in gone])
        twin = plugin(threaded)
        twin.set_scene(t.scene())
        nodes_equal(gpu, twin, name)
    print(results)
    assert results["alternating"][3] > 16, "more runs per plane than one copy launch of the append takes"
    assert results["one"][2] == results["alternating"][2] > 0


# ---------------------------------------------------------------------------------------------------------------- 3. in flight
@MODES
def test_a_removal_with_eight_frames_in_flight(threaded):
    gone = [0, 3, 6]
    left = [k for k in ALL if k not in gone]
    (d, _, ids), (w, _, _), (t, _, _) = build(ALL, left), build(ALL, left), build(left, left)
    gpu, with_, twin = plugin(threaded), plugin(threaded), plugin(threaded)
    cam, lights, s = view()
    gpu.set_scene(d.scene())
    with_.set_scene(w.scene())
    twin.set_scene(t.scene())
    for n in range(1, 9):
        gpu.render(cam, s, lights=lights, frame_number=n)   # (no wait in between)
    remove(gpu, d, ids, gone)
    assert gpu.engine.last_remove()[4] == 0
    frame8 = snapshot(gpu)
    for n in range(9, 12):
        gpu.render(cam, s, lights=lights, frame_number=n)
    for n in range(1, 9):
        with_.render(cam, s, lights=lights, frame_number=n)
        twin.render(cam, s, lights=lights, frame_number=n)
    assert diff_buffers(frame8, snapshot(with_)) == {}, "frame 8, read after the removal, differs from a run that kept the meshes"
    for n in range(9, 12):
        twin.render(cam, s, lights=lights, frame_number=n)
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad
    nodes_equal(gpu, twin, "in flight")


# ---------------------------------------------------------------------------------------------------------------- 4. survivors' state
def deformables(keep):
    """the meshes `keep`, mesh 1 instanced, and behind them a cloth (vertices updated), a second cloth (tree rebuilt), a cylinder (skinned)
    and a sphere (morphing): (builder, {name: dict(id, data...)})"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    ids = {k: b.add_mesh(*mesh_data(k)) for k in keep}
    b.add_instance(ids[1], mat, place(1))
    cp, cn, cuv, ci = S.cloth_grid(6, 5, size=1.5)
    yp, yn, yuv, yi, ji, jw = S.bending_cylinder()
    sp, sn, suv, si = S._sphere(5, 7)
    m = dict(cloth=dict(id=b.add_mesh(cp, cn, cuv, ci), rest=cp, normals=cn), cloth2=dict(id=b.add_mesh(cp + np.float32(0.02), cn, cuv, ci), rest=cp, normals=cn),
             cylinder=dict(id=b.add_mesh(yp, yn, yuv, yi), rest=yp, normals=yn, joints=ji, weights=jw), sphere=dict(id=b.add_mesh(sp, sn, suv, si), rest=sp, normals=sn))
    for k, name in enumerate(m):
        b.add_instance(m[name]["id"], mat, S._trs((0.9 * k - 1.2, 1.0, 0.4), (0.2, 0.3 * k, 0.0), (0.8, 0.8, 0.8)))
    b.finish()
    return b, ids, m


def deform(p, b, m, frame, first):
    e = p.engine
    index = {name: b.mesh_index(v["id"]) for name, v in m.items()}
    rng = np.random.default_rng(3)
    deltas = rng.normal(0.0, 0.05, (2,) + m["sphere"]["rest"].shape).astype(np.float32)
    if first:
        e.set_mesh_skin(index["cylinder"], m["cylinder"]["rest"], m["cylinder"]["normals"], m["cylinder"]["joints"], m["cylinder"]["weights"])
        e.set_mesh_morph_targets(index["sphere"], m["sphere"]["rest"], m["sphere"]["normals"], deltas)
    e.update_mesh_vertices(index["cloth"], *S.waving_cloth(m["cloth"]["rest"], frame, amplitude=0.15))
    e.update_mesh_vertices(index["cloth2"], *S.waving_cloth(m["cloth2"]["rest"], frame + 2, amplitude=0.1))
    if first:
        e.rebuild_mesh_tree(index["cloth2"], F.TREE_SAH)
    e.deform_meshes([("skin", index["cylinder"], S.bend_joints(frame)), ("morph", index["sphere"], np.array([0.3 * frame, 0.7], np.float32))])
    return index


@MODES
def test_survivors_keep_skins_morph_sets_deformed_vertices_and_rebuilt_trees(threaded):
    gone = [0, 2, 5]
    left = [k for k in ALL if k not in gone]
    (d, ids, m), (t, _, tm) = deformables(ALL), deformables(left)
    gpu, twin = plugin(threaded), plugin(threaded)
    cam, lights, s = view()
    for p, b, mm in ((gpu, d, m), (twin, t, tm)):
        p.set_scene(b.scene())
        deform(p, b, mm, 3, True)
        p.render(cam, s, lights=lights, frame_number=1)
    wide_before = gpu.engine.last_deform()[5]
    extents = [d.remove_mesh(ids[k]) for k in sorted(gone, reverse=True)]
    old = {name: d.mesh_extent(v["id"] - len(gone)) for name, v in m.items()}
    gpu.remove_meshes(extents)
    assert gpu.engine.last_remove()[4] == 0
    d.finish()
    for v in m.values():
        v["id"] -= len(gone)
    render_and_compare([gpu, twin], cam, s, lights, (2,), "the frame after the removal")
    if threaded:
        assert gpu.engine.last_deform()[5] == wide_before, "the frame after the removal derived wide records again"
    nodes_equal(gpu, twin, "deformed survivors")
    for p, b, mm in ((gpu, d, m), (twin, t, tm)):   # each deformed again, under its new record
        index = deform(p, b, mm, 5, False)
    for name in m:
        assert bytes(index[name]) == bytes(d.mesh_index(m[name]["id"])) and index[name].vertex < old[name].vertex
        g, w = gpu.engine.read_mesh_geometry(d.mesh_index(m[name]["id"])), twin.engine.read_mesh_geometry(index[name])
        for key in g:
            assert g[key].tobytes() == w[key].tobytes(), f"{key} of the {name} differ from the twin's after the second deformation"
    nodes_equal(gpu, twin, "deformed again")
    render_and_compare([gpu, twin], cam, s, lights, (3, 4), "deformed again")


# ---------------------------------------------------------------------------------------------------------------- 5. stale mirrors
@MODES
@pytest.mark.parametrize("how", ["refit", "device-poses"])
def test_a_removal_with_stale_mirrors_equals_the_twin_given_the_same_poses(threaded, how):
    import torch

    gone = [2, 3, 7]
    left = [k for k in ALL if k not in gone]
    (d, _, ids), (t, _, _) = build(ALL, left), build(left, left)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    twin.set_scene(t.scene())
    pose = S._trs((-0.7, 0.3, 0.2), (0.0, 0.5, 0.0), (1.0, 1.0, 1.0))
    models = torch.tensor(np.stack([np.asarray(place(k), np.float32).reshape(16) for k in left]), device="cuda")
    models[1] = torch.tensor(np.asarray(pose, np.float32).reshape(16), device="cuda")
    for p, b in ((gpu, d), (twin, t)):
        if how == "refit":
            b.set_instance_transform(1, pose)
            assert p.engine.refit_instances(b) == 1
        else:
            p.set_instance_transforms(b, models)
    remove(gpu, d, ids, gone)
    assert gpu.engine.last_remove()[4] == 0
    nodes_equal(gpu, twin, how)
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), how)


# ---------------------------------------------------------------------------------------------------------------- 6. / 7. what follows
@MODES
def test_an_add_after_a_removal_finds_room_and_instances_follow(threaded):
    gone = [0, 6, 7]
    left = [k for k in ALL if k not in gone]
    (d, mat, ids), (t, _, _) = build(), build(left, left)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    builds = mesh_builds(gpu)
    remove(gpu, d, ids, gone, ALL)
    p, _, i = soup(333, 41)
    new = [add(b, how, p, i) for b, how in ((d, "device"), (t, "twin"))]
    assert new[0] == new[1] == len(left)
    d.finish()
    gpu.add_meshes(d)
    assert gpu.engine.last_add()[:2] == (1, 333) and gpu.engine.last_add()[4] == 0, "the add after the removal moved the scene again"
    for b in (d, t):
        b.add_instance(new[0], mat, place(9))
        b.add_instance(1, mat, place(11))   # ... and one more of a survivor, named by its new id
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    assert mesh_builds(gpu) == builds
    twin.set_scene(t.finish())
    survivors_equal(gpu, twin, t, len(left) + 1, "remove, add, instances")
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "remove, add, instances")


@MODES
def test_an_instance_of_a_survivor_added_after_the_removal(threaded):
    gone = [2, 5]
    left = [k for k in ALL if k not in gone]
    (d, mat, ids), (t, _, _) = build(ALL, left), build(left, left)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    builds = mesh_builds(gpu)
    remove(gpu, d, ids, gone)
    for b in (d, t):
        b.add_instance(len(left) - 1, mat, place(12))   # the mesh of 1 025 triangles, behind both removed ones
        b.add_instance(2, mat, place(13))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    assert mesh_builds(gpu) == builds, "the rebased mirror did not match the builder's records: the mesh level was laid out again"
    twin.set_scene(t.finish())
    survivors_equal(gpu, twin, t, len(left), "an instance after the removal")
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "an instance after the removal")


# ---------------------------------------------------------------------------------------------------------------- 8. small scene
@MODES
def test_cornell_takes_the_full_layout_and_refuses_it_after_a_deformation(threaded):
    def cornell(extra):
        scene = hk.load_cornell()
        b = scene.builder
        m = add(b, "twin", *soup(20, 8)[::2], deferred=False) if extra else None
        b.finish()
        return b, m

    (d, m), (t, _) = cornell(True), cornell(False)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    twin.set_scene(t.scene())
    gpu.remove_meshes([d.remove_mesh(m)])
    assert gpu.engine.last_remove()[:2] == (1, 20) and gpu.engine.last_remove()[4] == 1
    d.finish()
    nodes_equal(gpu, twin, "cornell")
    assert gpu.engine.traversal_mode() == twin.engine.traversal_mode()
    cam, s = hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS)
    render_and_compare([gpu, twin], cam, s, None, (1, 2), "cornell")
    # after a deformation the re-layout is refused, and nothing has changed
    (d, m), (k, _) = cornell(True), cornell(True)
    gpu, control = plugin(threaded), plugin(threaded)
    for p, b in ((gpu, d), (control, k)):
        p.set_scene(b.scene())
        index = b.mesh_index(0)
        rest = p.engine.read_mesh_geometry(index)["positions"]
        p.engine.update_mesh_vertices(index, rest * np.float32(0.97))
    e = d.remove_mesh(m)
    assert gpu.engine.api.raw("remove_meshes")(gpu.engine.ctx, C.byref(e), 1) == F.HK_E_NOT_READY
    nodes_equal(gpu, control, "cornell, refused")
    render_and_compare([gpu, control], cam, s, None, (1,), "cornell, refused")


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
@MODES
def test_refusals_enqueue_nothing(threaded):
    left = [k for k in ALL if k != 6]
    (d, _, ids), (k_, _, _) = build(), build()
    gpu, control, empty = plugin(threaded), plugin(threaded), plugin(threaded)
    api, ctx = gpu.engine.api, gpu.engine.ctx
    call = api.raw("remove_meshes")
    good = d.mesh_extent(ids[2])
    assert call(empty.engine.ctx, C.byref(good), 1) == F.HK_E_NOT_READY   # no scene
    for p, b in ((gpu, d), (control, k_)):
        p.set_scene(b.scene())
        pos, nrm = mesh_data(6)[:2]   # a skin makes the mesh of 300 triangles a mesh the context knows beyond its instance
        p.engine.set_mesh_skin(b.mesh_index(6), pos, nrm, np.zeros((len(pos), 4), np.uint16), np.tile(np.array([1, 0, 0, 0], np.float32), (len(pos), 1)))
        # a ray query derives, in default mode, the wide records of every instanced mesh: the mesh of 40 triangles, which then loses its
        # instance and has no skin, stays a mesh the context knows through them alone
        p.engine.cast_rays(make_rays(np.array([[0.0, 0.5, 4.0]], np.float32), np.array([[0.0, 0.0, -1.0]], np.float32)))
        b.remove_instance(6)
        b.remove_instance(5)
        p.engine.update_instances_on_device(b, F.TREE_SAH)
    before = bytes(gpu.engine.read_mesh_nodes()[0])
    stats = gpu.engine.stats()
    counters = (stats.scene_mesh_builds, stats.scene_instance_builds, stats.scene_async_instance_uploads)

    def ext(e, **changes):
        out = F.HkMeshExtent(e.vertex, e.n_vertices, e.primitive, e.n_primitives, e.node_offset, e.node_count)
        for key, v in changes.items():
            setattr(out, key, v)
        return out

    def refused(*extents, entry=None):
        arr = (F.HkMeshExtent * len(extents))(*extents)
        assert call(ctx, arr, len(extents)) == F.HK_E_INVALID, api.last_error()
        if entry is not None:
            assert f"entry {entry}:" in api.last_error(), api.last_error()

    free = d.mesh_extent(ids[6])   # no instance names it any more
    other = d.mesh_extent(ids[7])
    assert call(None, C.byref(free), 1) == F.HK_E_INVALID
    assert call(ctx, None, 1) == F.HK_E_INVALID
    refused(ext(free, node_offset=2**31), entry=0)                                   # leaves the mirrors
    refused(ext(free, vertex=2**32 - 10), entry=0)
    refused(ext(free, n_primitives=0, node_count=1), entry=0)
    refused(ext(free, node_count=free.node_count + 1), entry=0)                      # not 3 n - 2
    refused(free, ext(free, n_primitives=10, node_count=28), entry=1)                # two that overlap
    refused(free, free, entry=1)
    refused(free, ext(other, vertex=free.vertex - 5, n_vertices=5), entry=1)         # ordered differently in vertices and nodes
    refused(good, entry=0)                                                           # an instance still uses the mesh
    assert "instance" in api.last_error()
    refused(free, other, entry=1)
    refused(ext(other, n_primitives=100, node_count=298, n_vertices=10), entry=0)    # ... or a part of it
    assert "instance" in api.last_error()
    refused(ext(free, n_primitives=100, node_count=298, n_vertices=10), entry=0)     # cuts a mesh the context knows: a deformable mesh
    assert "cuts the deformable mesh" in api.last_error()
    if threaded:   # ... a mesh with wide records (the exact walk keeps none: there the context knows nothing of a mesh without instance or skin)
        plain = d.mesh_extent(ids[5])
        refused(ext(plain, n_primitives=10, node_count=28, n_vertices=10), entry=0)
        assert "cuts the mesh tree" in api.last_error()
        refused(free, ext(plain, node_offset=plain.node_offset + 3, primitive=plain.primitive + 1, n_primitives=10, node_count=28, n_vertices=10), entry=1)
        assert "cuts the mesh tree" in api.last_error()
    refused(ext(free, node_offset=free.node_offset + 3, primitive=free.primitive + 1, n_primitives=100, node_count=298, n_vertices=10), entry=0)
    # nothing to do: HK_OK, nothing enqueued
    assert call(ctx, None, 0) == F.HK_OK
    assert call(ctx, C.byref(ext(free, node_count=0)), 1) == F.HK_OK and gpu.engine.last_remove() == (0, 0, 0, 0, 0, 0)
    assert api.raw("multi_remove_meshes")(None, C.byref(free), 1) == F.HK_E_INVALID
    stats = gpu.engine.stats()
    assert counters == (stats.scene_mesh_builds, stats.scene_instance_builds, stats.scene_async_instance_uploads)
    assert bytes(gpu.engine.read_mesh_nodes()[0]) == before
    cam, lights, s = view()
    render_and_compare([gpu, control], cam, s, lights, (1, 2), "after the refusals")
    # ... and the extent itself is accepted
    gpu.remove_meshes([d.remove_mesh(ids[6])])
    report = gpu.engine.last_remove()
    assert report[:2] == (1, 300)
    # a refused call leaves the report of the last removal as it was; a call with nothing to do clears it
    # (the mesh of 1 025 triangles where it lies now, its instance still there: refused by the last but one of the checks)
    refused(ext(other, vertex=other.vertex - free.n_vertices, primitive=other.primitive - free.n_primitives, node_offset=other.node_offset - free.node_count), entry=0)
    assert "instance" in api.last_error()
    assert call(ctx, None, 1) == F.HK_E_INVALID and gpu.engine.last_remove() == report


# ---------------------------------------------------------------------------------------------------------------- 10. bands
@MODES
def test_bands_removing_equal_the_single_context(threaded):
    from bevy_hikari_amd.distributed import MultiEngine

    gone = [0, 4, 5]
    left = [k for k in ALL if k not in gone]
    (d, _, ids), (r, _, rids) = build(ALL, left), build(ALL, left)
    flags = F.CTX_DETERMINISTIC_SCATTER
    s = hk.HikariSettings(**SETTINGS)
    w, h = 96, 64
    cam, lights = synthetic_camera(w, h), hk.lights_uniform(directional=SUN)
    v, pv = cam.view_uniform(), cam.previous_view_uniform()
    if threaded:
        with product_default_traversal():
            m, ref = MultiEngine([0, 0], flags=flags), hk.Engine(device=0, flags=flags)
    else:
        m, ref = MultiEngine([0, 0], flags=flags), hk.Engine(device=0, flags=flags)
    m.upload_noise(); ref.upload_noise()
    m.upload_scene(d.scene()); ref.upload_scene(r.scene())
    m.resize(w, h, 1.0); ref.resize(w, h, 1.0)
    m.set_band_bounds([0, 20, 64])
    f = hk.frame_uniform(s, 1)
    m.frame_render(f, v, pv, lights, s.to_c()); ref.frame_render(f, v, pv, lights, s.to_c())
    m.remove_meshes([d.remove_mesh(ids[k]) for k in sorted(gone, reverse=True)])
    ref.remove_meshes([r.remove_mesh(rids[k]) for k in sorted(gone, reverse=True)])
    assert all(e.last_remove()[:2] == (3, 7 + 3 + 40) and e.last_remove()[4] == 0 for e in m.contexts)
    want = bytes(ref.read_mesh_nodes()[0])
    for k, e in enumerate(m.contexts):
        assert bytes(e.read_mesh_nodes()[0]) == want, f"band {k}: mesh-level nodes differ from the single context's"
    for n in range(2, 4):
        f = hk.frame_uniform(s, n)
        m.frame_render(f, v, pv, lights, s.to_c())
        ref.frame_render(f, v, pv, lights, s.to_c())
        m.wait(); ref.wait()
        for buf in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_VELOCITY_UV, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(buf).view(np.uint8) == ref.read(buf).view(np.uint8)).all(), f"frame {n}: buffer {buf} differs"


# ---------------------------------------------------------------------------------------------------------------- 11. ray queries
@MODES
def test_ray_queries_after_a_removal_equal_the_twins(threaded):
    gone = [0, 2, 3, 6]
    left = [k for k in ALL if k not in gone]
    (d, _, ids), (t, _, _) = build(), build(left, left)
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    twin.set_scene(t.scene())
    rng = np.random.default_rng(21)
    origins = rng.uniform(-3.0, 3.0, (4096, 3)).astype(np.float32)
    targets = rng.uniform(-1.0, 1.5, (4096, 3)).astype(np.float32)
    rays = make_rays(origins, targets - origins)
    gpu.engine.cast_rays(rays)   # (a query before the removal: in default mode its wide records are the ones that move)
    remove(gpu, d, ids, gone, ALL)
    got, want = gpu.engine.cast_rays(rays, attributes=True), twin.engine.cast_rays(rays, attributes=True)
    assert (want["status"] == F.RAY_HIT).sum() > 100
    assert got.tobytes() == want.tobytes(), "closest hits differ from the twin's"
    got, want = gpu.engine.cast_rays(rays, any_hit=True), twin.engine.cast_rays(rays, any_hit=True)
    assert (got["status"] == want["status"]).all(), "occlusion differs from the twin's"
