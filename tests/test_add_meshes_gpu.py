"""hk_add_meshes: meshes added to a loaded scene on the device.  A context that loaded a base scene and then received meshes through
hk_add_meshes must hold, byte for byte, what a fresh context holds after hk_upload_scene of the twin builder that had every mesh from
the start (add_mesh + hk_scene_builder_rebuild_mesh_tree for what was deferred, as tests/test_scene_load_gpu.py builds its twins).  The
base scene lies beyond the LDS copy; every case runs with the product's default traversal (8 orderings) and under the suite's
HK_CTX_EXACT_TRAVERSAL (1 ordering, two slots)."""
import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from test_mesh_deform_gpu import SETTINGS, frame_data
from test_mesh_rebuild import IDENTITY, NODE, flat
from test_mesh_rebuild_gpu import SIZED, soup
from test_scene_load_gpu import assert_builders_equal, nodes_equal, render_and_compare

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("threaded", [False, True], ids=["exact", "default"])
SUN = dict(color=(1.0, 0.96, 0.9), illuminance=20000.0, direction_to_light=(0.35, 0.8, 0.45))


def plugin(threaded):
    """default: the product's traversal (threaded trees, the wide walk); exact: the suite's reference walk.  Both resolve the reference's
    scatter race in all three channels: some cases move instances, and the channels without a reader race by design otherwise."""
    if threaded:
        with product_default_traversal():
            return hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    return hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)


def place(k):
    return S._trs((0.45 * (k % 5) - 0.9, 0.4 + 0.35 * (k // 5), 0.3 * (k % 3) - 0.3), (0.0, 0.37 * k, 0.0), (0.5, 0.5, 0.5))


def base_builder():
    """a 1 100-triangle soup, a cloth and a sphere, one instance each: (finished builder, material id, mesh ids)"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    p, _, i = soup(1100, 11)
    n, uv = flat(p)
    ids = [b.add_mesh(p, n, uv, i)]
    p, n, uv, i = S.cloth_grid(5, 4)
    ids.append(b.add_mesh(p, n, uv, i))
    p, n, uv, i = S._sphere(5, 6)
    ids.append(b.add_mesh(p, n, uv, i))
    for k, m in enumerate(ids):
        b.add_instance(m, mat, S._trs((1.1 * k - 1.0, 0.0, 0.0), (0.0, 0.2 * k, 0.0), (1.0, 1.0, 1.0)))
    b.finish()
    return b, mat, ids


def add(b, how, positions, idx, deferred=True):
    """one mesh as the device run adds it (how='device': deferred where `deferred`) or as the twin does (add_mesh + rebuild_mesh_tree)"""
    n, uv = flat(positions)
    m = b.add_mesh(positions, n, uv, idx, build_tree=not (deferred and how == "device"))
    if deferred and how == "twin":
        b.rebuild_mesh_tree(m)
    return m


def the_nine(b, how):
    """deferred meshes of 1, 2, 3, 1023, 1024 and 1025 triangles and the whole-chip half split, two meshes whose trees the host built"""
    ids = [add(b, how, SIZED[name][0], SIZED[name][2]) for name in ("1", "2", "3", "1023", "1024", "1025", "half_split_40000")]
    p, _, i = soup(300, 91)
    ids.append(add(b, how, p, i, deferred=False))
    p, _, _, i = S._sphere(6, 7)
    ids.append(add(b, how, p, i, deferred=False))
    return ids


def small(b, how, k, triangles=40):
    p, _, i = soup(triangles, 500 + k)
    return add(b, how, p, i)


def geometry_equal(gpu, twin, b, ids, what):
    for m in ids:
        index = b.mesh_index(m)
        g, t = gpu.engine.read_mesh_geometry(index), twin.engine.read_mesh_geometry(index)
        for key in ("positions", "normals", "triangles", "box"):
            assert g[key].tobytes() == t[key].tobytes(), f"{what}: {key} of mesh {m} differ from the twin's"


def view():
    return synthetic_camera(96, 64), hk.lights_uniform(directional=SUN), hk.HikariSettings(**SETTINGS)


def mesh_builds(p):
    return p.engine.stats().scene_mesh_builds


# ---------------------------------------------------------------------------------------------------------------- 1. equal to the twin
@MODES
def test_added_meshes_equal_the_uploaded_twin(threaded):
    (d, mat, base_ids), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    _, _, orderings = gpu.engine.read_mesh_nodes()   # (lays the scene out)
    assert orderings == (8 if threaded else 1)
    builds, device_builds = mesh_builds(gpu), gpu.engine.stats().scene_device_tree_builds
    ids, tids = the_nine(d, "device"), the_nine(t, "twin")
    assert ids == tids
    d.finish()
    t.finish()
    assert d.pending_mesh_trees() == 7
    gpu.add_meshes(d, F.TREE_SAH)
    assert d.pending_mesh_trees() == 0
    assert_builders_equal(d, t, "after the add")
    meshes, tris, launches, on_host, relocated = gpu.engine.last_add()
    print(f"add: {meshes} meshes / {tris} triangles in {launches} launches, {on_host} laid out by the host, relocated {relocated}")
    assert (meshes, tris, on_host, relocated) == (7, 1 + 2 + 3 + 1023 + 1024 + 1025 + 40000, 2, 1) and launches >= 4
    for b in (d, t):
        for k, m in enumerate(ids):
            b.add_instance(m, mat, place(k))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    twin.set_scene(t.finish())
    assert nodes_equal(gpu, twin, "the nine")[1] == orderings
    geometry_equal(gpu, twin, t, base_ids + ids, "the nine")
    assert mesh_builds(gpu) == builds, "the append laid the mesh level out again on the host"
    assert gpu.engine.stats().scene_device_tree_builds >= device_builds + 7
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "the nine")
    assert mesh_builds(gpu) == builds


@MODES
def test_forty_small_meshes_take_no_more_launches_than_four(threaded):
    counts = {}
    for n in (40, 4):
        b, _, _ = base_builder()
        p = plugin(threaded)
        p.set_scene(b.scene())
        for k in range(n):
            small(b, "device", k, triangles=(1, 2, 7, 64, 511)[k % 5])
        b.finish()
        p.add_meshes(b)
        counts[n] = p.engine.last_add()
        assert counts[n][0] == n and counts[n][3] == 0
    print(f"40 meshes: {counts[40][2]} launches, 4 meshes: {counts[4][2]}")
    assert counts[40][2] <= counts[4][2], counts


# ---------------------------------------------------------------------------------------------------------------- 2. instanced later
@MODES
def test_a_mesh_instanced_two_updates_after_the_add(threaded):
    """The twin context holds every mesh from the start (hk_upload_scene) and takes the same three instance updates and frames."""
    (d, mat, _), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    late, first = small(d, "device", 0, 700), small(d, "device", 1, 90)
    assert (late, first) == (small(t, "twin", 0, 700), small(t, "twin", 1, 90))
    d.finish()
    gpu.add_meshes(d)
    twin.set_scene(t.finish())
    builds = mesh_builds(gpu)
    cam, lights, s = view()
    for update, meshes in enumerate(([first], [], [late])):
        for b in (d, t):
            for m in meshes:
                b.add_instance(m, mat, place(3 + m))
            b.set_instance_transform(0, S._trs((-1.0, 0.1 * (update + 1), 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
        for p, b in ((gpu, d), (twin, t)):
            p.engine.update_instances_on_device(b, F.TREE_SAH)
            p.render(cam, s, lights=lights, frame_number=update + 1)
        assert mesh_builds(gpu) == builds, f"update {update}: the mesh level was laid out again"
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad
    nodes_equal(gpu, twin, "instanced later")


# ---------------------------------------------------------------------------------------------------------------- 3. growth
@MODES
def test_six_adds_relocate_at_most_once(threaded):
    (d, mat, base_ids), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    raw, count, orderings = gpu.engine.read_mesh_nodes()
    earlier = np.frombuffer(bytes(raw), NODE).reshape(orderings, count).copy()
    ids = []
    for k in range(6):
        ids.append(small(d, "device", k, 60 + k))
        assert small(t, "twin", k, 60 + k) == ids[-1]
        d.finish()
        gpu.add_meshes(d)
        last = gpu.engine.last_add()
        assert last[:2] == (1, 60 + k) and (k == 0 or last[4] == 0), (k, last)
        raw, count, orderings = gpu.engine.read_mesh_nodes()
        now = np.frombuffer(bytes(raw), NODE).reshape(orderings, count).copy()
        assert now[:, :earlier.shape[1]].tobytes() == earlier.tobytes(), f"add {k}: the nodes of earlier meshes changed"
        earlier = now
    for b in (d, t):
        for k, m in enumerate(ids):
            b.add_instance(m, mat, place(k))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    twin.set_scene(t.finish())
    nodes_equal(gpu, twin, "six adds")
    geometry_equal(gpu, twin, t, base_ids + ids, "six adds")
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "six adds")


# ---------------------------------------------------------------------------------------------------------------- 4. in flight
@MODES
def test_an_add_that_relocates_with_eight_frames_in_flight(threaded):
    (d, mat, _), (t, _, _), (plain, _, _) = base_builder(), base_builder(), base_builder()
    gpu, twin, without = plugin(threaded), plugin(threaded), plugin(threaded)
    cam, lights, s = view()
    gpu.set_scene(d.scene())
    without.set_scene(plain.scene())
    ids = [small(b, how, 0, 900) for b, how in ((d, "device"), (t, "twin"))]
    d.finish()
    t.finish()
    twin.set_scene(t.scene())   # every mesh from the start, the new one without an instance yet
    for n in range(1, 9):
        gpu.render(cam, s, lights=lights, frame_number=n)   # (no wait in between)
    gpu.add_meshes(d)
    assert gpu.engine.last_add()[4] == 1
    frame8 = snapshot(gpu)
    for b in (d, t):
        b.add_instance(ids[0], mat, place(2))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    for n in range(9, 13):
        gpu.render(cam, s, lights=lights, frame_number=n)
    for n in range(1, 9):
        without.render(cam, s, lights=lights, frame_number=n)
        twin.render(cam, s, lights=lights, frame_number=n)
    assert diff_buffers(frame8, snapshot(without)) == {}, "frame 8, read after the add, differs from a run without the add"
    twin.engine.update_instances_on_device(t, F.TREE_SAH)
    for n in range(9, 13):
        twin.render(cam, s, lights=lights, frame_number=n)
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad


# ---------------------------------------------------------------------------------------------------------------- 5. device state kept
@MODES
def test_deformations_skins_and_rebuilt_trees_survive_an_add(threaded):
    """`control` does everything but the add"""
    plugins, scenes = [], []
    for _ in range(2):
        scene, sun, meshes = S.deforming_scene("yard")
        p = plugin(threaded)
        p.set_scene(scene)
        cl, cy = meshes["cloth"], meshes["cylinder"]
        data, joints = frame_data(meshes, 3)
        p.engine.update_mesh_vertices(cl["index"], *data["cloth"])
        p.engine.rebuild_mesh_tree(cl["index"], F.TREE_SAH)
        p.engine.set_mesh_skin(cy["index"], cy["rest"], cy["normals"], cy["joints"], cy["weights"])
        plugins.append(p)
        scenes.append(scene)
    gpu, control = plugins
    e, b = gpu.engine, scenes[0].builder
    before = e.read_mesh_geometry(cl["index"])
    raw, count, orderings = e.read_mesh_nodes()
    lo, hi = cl["index"].node_offset, cl["index"].node_offset + cl["index"].node_count
    nodes_before = np.frombuffer(bytes(raw), NODE).reshape(orderings, count)[:, lo:hi].tobytes()
    small(b, "device", 0, 333)
    b.finish()
    gpu.add_meshes(b)
    assert e.last_add()[:2] == (1, 333) and e.last_add()[4] == 1
    after = e.read_mesh_geometry(cl["index"])
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), f"{key} of the deformed mesh changed with the add"
    raw, count, orderings = e.read_mesh_nodes()
    assert np.frombuffer(bytes(raw), NODE).reshape(orderings, count)[:, lo:hi].tobytes() == nodes_before
    for p in plugins:   # the skin set before the add is still there
        p.engine.skin_mesh(cy["index"], joints)
    got, want = e.read_mesh_geometry(cy["index"]), control.engine.read_mesh_geometry(cy["index"])
    for key in got:
        assert got[key].tobytes() == want[key].tobytes(), f"{key} of the skinned mesh differ from the run without the add"
    # ... and instance-set updates stay refused in that state, as before the add
    assert e.api.raw("update_scene_instances")(e.ctx, b.h, F.TREE_SAH) == F.HK_E_NOT_READY
    cam, s = synthetic_camera(96, 64), hk.HikariSettings(**SETTINGS)
    render_and_compare(plugins, cam, s, hk.lights_uniform(directional=sun), (1, 2), "after an add on a deformed scene")


@MODES
def test_an_add_after_a_refit_equals_the_twin_given_the_same_poses(threaded):
    (d, mat, _), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    pose = S._trs((-0.7, 0.3, 0.2), (0.0, 0.5, 0.0), (1.0, 1.0, 1.0))
    d.set_instance_transform(1, pose)
    assert gpu.engine.refit_instances(d) == 1
    ids = [small(b, how, 0, 450) for b, how in ((d, "device"), (t, "twin"))]
    d.finish()
    gpu.add_meshes(d)
    for b in (d, t):
        b.add_instance(ids[0], mat, place(1))
    t.set_instance_transform(1, pose)
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    t.finish()
    twin.set_scene(t.finish())   # (twice: nothing moves between the last two finishes, as on the device)
    nodes_equal(gpu, twin, "after a refit")
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "after a refit")


# ---------------------------------------------------------------------------------------------------------------- 6. small scene
@pytest.mark.parametrize("triangles", [2, 2000])
@MODES
def test_cornell_takes_the_full_layout(threaded, triangles):
    dev, tw = hk.load_cornell(), hk.load_cornell()
    d, t = dev.builder, tw.builder
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(dev)
    gpu.engine.read_mesh_nodes()
    ids = [small(b, how, 0, triangles) for b, how in ((d, "device"), (t, "twin"))]
    d.finish()
    gpu.add_meshes(d)
    assert gpu.engine.last_add()[:2] == (1, triangles) and gpu.engine.last_add()[4] == 0
    pose = S._trs((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.3, 0.3, 0.3))
    for b in (d, t):
        b.add_instance(ids[0], 0, pose)
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    t.finish()
    twin.set_scene(t.finish())
    nodes_equal(gpu, twin, f"cornell + {triangles}")
    assert gpu.engine.traversal_mode() == twin.engine.traversal_mode()
    render_and_compare([gpu, twin], hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS), None, (1, 2), f"cornell + {triangles}")


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
@MODES
def test_refusals_write_nothing(threaded):
    (d, mat, _), (other, _, _), (plain, _, _) = base_builder(), base_builder(), base_builder()
    gpu, control, empty = plugin(threaded), plugin(threaded), plugin(threaded)
    api, ctx = gpu.engine.api, gpu.engine.ctx
    small(d, "device", 0, 200)
    d.finish()
    assert api.raw("add_meshes")(empty.engine.ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY   # no scene
    gpu.set_scene(plain.scene())
    control.set_scene(plain.scene())
    before = bytes(gpu.engine.read_mesh_nodes()[0])
    stats = gpu.engine.stats()
    counters = (stats.scene_mesh_builds, stats.scene_instance_builds, stats.scene_async_instance_uploads, stats.scene_device_tree_builds)
    assert api.raw("add_meshes")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("add_meshes")(ctx, None, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("add_meshes")(ctx, d.h, 2) == F.HK_E_INVALID
    # a builder whose existing meshes are not the context's: a larger first mesh, and one that holds less than the context
    p, _, i = soup(1101, 11)
    n, uv = flat(p)
    stranger = SceneBuilder()
    stranger.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    stranger.add_instance(stranger.add_mesh(p, n, uv, i), 0, IDENTITY)
    small(stranger, "device", 0, 200)
    stranger.finish()
    assert api.raw("add_meshes")(ctx, stranger.h, F.TREE_SAH) == F.HK_E_INVALID
    assert "not the context's" in api.last_error()
    unfinished = SceneBuilder()
    assert api.raw("add_meshes")(ctx, unfinished.h, F.TREE_SAH) == F.HK_E_NOT_READY
    d.finish(build_trees=False)   # stand-in instance trees (hk_scene_builder_finish_instances)
    assert api.raw("add_meshes")(ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY
    d.finish()
    small(other, "device", 0, 200)   # added, not finished
    assert api.raw("add_meshes")(ctx, other.h, F.TREE_SAH) == F.HK_E_NOT_READY
    assert api.raw("multi_add_meshes")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    # nothing new: HK_OK, nothing enqueued
    assert api.raw("add_meshes")(ctx, plain.h, F.TREE_SAH) == F.HK_OK
    assert gpu.engine.last_add() == (0, 0, 0, 0, 0)
    stats = gpu.engine.stats()
    assert counters == (stats.scene_mesh_builds, stats.scene_instance_builds, stats.scene_async_instance_uploads, stats.scene_device_tree_builds)
    assert bytes(gpu.engine.read_mesh_nodes()[0]) == before and d.pending_mesh_trees() == 1
    cam, lights, s = view()
    render_and_compare([gpu, control], cam, s, lights, (1, 2), "after the refusals")
    # a deferred mesh above the device limit (lowered through the debug option) is completed by the host inside the call
    t, _, _ = base_builder()
    small(t, "twin", 0, 200)
    gpu.engine.set_debug_option(F.DEBUG_OPT_LOAD_DEVICE_LIMIT, 100)
    gpu.add_meshes(d)
    assert gpu.engine.last_add()[:4] == (0, 0, 0, 1) and d.pending_mesh_trees() == 0
    t.finish()
    assert_builders_equal(d, t, "host completion inside the add")
    # the full layout of a one-slot scene is refused while the mirrors are stale (instances refit on the device)
    cornell = hk.load_cornell()
    lds = plugin(threaded)
    lds.set_scene(cornell)
    b = cornell.builder
    b.set_instance_transform(0, S._trs((0.0, 0.05, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    assert lds.engine.refit_instances(b) == 1
    small(b, "device", 0, 2)
    b.finish()
    assert api.raw("add_meshes")(lds.engine.ctx, b.h, F.TREE_SAH) == F.HK_E_NOT_READY and b.pending_mesh_trees() == 1


# ---------------------------------------------------------------------------------------------------------------- 8. bands
@MODES
def test_bands_adding_equal_the_single_context(threaded):
    from bevy_hikari_amd.distributed import MultiEngine

    (d, mat, _), (r, _, _) = base_builder(), base_builder()
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
    for b in (d, r):
        ids = [small(b, "device", 0, 500), small(b, "device", 1, 3)]
        p, _, i = soup(120, 77)
        ids.append(add(b, "device", p, i, deferred=False))
        b.finish()
    m.add_meshes(d, F.TREE_SAH)
    ref.add_meshes(r, F.TREE_SAH)
    assert d.pending_mesh_trees() == 0 and m.contexts[0].last_add()[:2] == (2, 503) and m.contexts[1].last_add()[0] == 0 and m.contexts[1].last_add()[3] == 3
    for b in (d, r):
        for k, mesh in enumerate(ids):
            b.add_instance(mesh, mat, place(k))
    m.update_instances_on_device(d, F.TREE_SAH)
    ref.update_instances_on_device(r, F.TREE_SAH)
    want = bytes(ref.read_mesh_nodes()[0])
    for k, e in enumerate(m.contexts):
        assert bytes(e.read_mesh_nodes()[0]) == want, f"band {k}: mesh-level nodes differ from the single context's"
    for n in range(1, 3):
        f = hk.frame_uniform(s, n)
        m.frame_render(f, v, pv, lights, s.to_c())
        ref.frame_render(f, v, pv, lights, s.to_c())
        m.wait(); ref.wait()
        for buf in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(buf).view(np.uint8) == ref.read(buf).view(np.uint8)).all(), f"frame {n}: buffer {buf} differs"


# ---------------------------------------------------------------------------------------------------------------- 9. materials
@MODES
def test_materials_appended_after_the_load_travel_with_the_instances(threaded):
    (d, _, _), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    gpu.set_scene(d.scene())
    gpu.engine.read_mesh_nodes()
    builds = mesh_builds(gpu)
    for b, how in ((d, "device"), (t, "twin")):
        a, c = small(b, how, 0, 150), small(b, how, 1, 64)
        if how == "device":
            b.finish()
            gpu.add_meshes(b)
        glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
        matte = b.add_material(S.standard_material((0.2, 0.6, 0.3, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
        b.add_instance(a, glow, place(1))
        b.add_instance(c, matte, place(2))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    assert mesh_builds(gpu) == builds
    twin.set_scene(t.finish())
    nodes_equal(gpu, twin, "appended materials")
    rec, alias = gpu.engine.read_emitters()
    trec, talias = twin.engine.read_emitters()
    assert len(rec) == 1 and rec.tobytes() == trec.tobytes() and alias.tobytes() == talias.tobytes()
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "appended materials")
    # a texture id at or above the uploaded texture count is refused
    bad = S.standard_material((0.5, 0.5, 0.5, 1.0), (0, 0, 0), 0.5, 0.0, 0.5)
    bad.base_color_texture = 3
    d.add_instance(0, d.add_material(bad), place(4))
    assert gpu.engine.api.raw("update_scene_instances")(gpu.engine.ctx, d.h, F.TREE_SAH) == F.HK_E_INVALID


# ---------------------------------------------------------------------------------------------------------------- 10. the uv plane
@MODES
def test_textured_meshes_keep_their_uvs_through_an_add_and_a_relocation(threaded):
    """The uv plane reaches the G-buffer (velocity_uv) and, through a texture, the albedo: a base cloth (its uvs are MOVED by the relocation) and an added cloth (its uvs are
    written by the append) carry a noise texture sampled at the nearest texel, so a uv that is off by anything shows in the albedo."""
    rng = np.random.default_rng(12)
    texels = rng.integers(0, 256, (2, 32, 32, 4), dtype=np.uint8)
    textures = [dict(rgba=texels[k], srgb=True, linear=False) for k in range(2)]
    textured = S.standard_material((1.0, 1.0, 1.0, 1.0), (0, 0, 0), 0.8, 0.0, 0.5)
    textured.base_color_texture = 0
    textured_too = S.standard_material((1.0, 1.0, 1.0, 1.0), (0, 0, 0), 0.8, 0.0, 0.5)
    textured_too.base_color_texture = 1
    (d, _, base_ids), (t, _, _) = base_builder(), base_builder()
    gpu, twin = plugin(threaded), plugin(threaded)
    for b in (d, t):
        tex, tex_too = b.add_material(textured), b.add_material(textured_too)
        b.set_instance_material(1, tex)   # the base cloth
        b.set_instance_transform(1, S._trs((0.0, 0.6, 0.0), (0.9, 0.0, 0.0), (2.2, 2.2, 2.2)))
    scene = d.finish()
    scene.textures = textures
    gpu.set_scene(scene)
    gpu.engine.read_mesh_nodes()
    builds = mesh_builds(gpu)
    p, n, uv, i = S.cloth_grid(7, 6)
    assert np.ptp(uv[:, 0]) > 0 and np.ptp(uv[:, 1]) > 0 and not np.array_equal(uv[:, 0], uv[:, 1])
    ids = []
    for b, how in ((d, "device"), (t, "twin")):
        m = b.add_mesh(p, n, uv, i, build_tree=how != "device")
        if how == "twin":
            b.rebuild_mesh_tree(m)
        ids.append(m)
    d.finish()
    gpu.add_meshes(d)
    assert gpu.engine.last_add()[4] == 1
    for b in (d, t):
        b.add_instance(ids[0], tex_too, S._trs((0.3, 1.4, 0.4), (1.2, 0.3, 0.0), (1.2, 1.2, 1.2)))
    gpu.engine.update_instances_on_device(d, F.TREE_SAH)
    t.finish()
    twin_scene = t.finish()
    twin_scene.textures = textures
    twin.set_scene(twin_scene)
    assert mesh_builds(gpu) == builds
    cam, lights, s = view()
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "textured")
    # both cloths are in view (the material id of the G-buffer tells them apart), with many uvs and many texels of their textures
    albedo = gpu.engine.read(F.BUF_ALBEDO)
    albedo = albedo.reshape(-1, albedo.shape[-1])
    material = np.ascontiguousarray(gpu.engine.read(F.BUF_INSTANCE_MATERIAL)).view(np.float32).reshape(-1, 2)[:, 1]
    uvs = np.ascontiguousarray(gpu.engine.read(F.BUF_VELOCITY_UV)).view(np.float32).reshape(-1, 4)[:, 2:]
    for name, mat in (("base", tex), ("added", tex_too)):
        seen = material == mat + 0.5
        n_uv, n_albedo = len(np.unique(uvs[seen], axis=0)), len(np.unique(albedo[seen], axis=0))
        print(f"{name} cloth: {int(seen.sum())} px, {n_uv} distinct uvs, {n_albedo} distinct albedo values")
        assert seen.sum() > 50 and n_uv > 50 and n_albedo > 8, f"the {name} cloth does not show its uvs and its texture"
