"""hk_load_scene: the trees of deferred meshes (hk_scene_builder_add_mesh_deferred) built on the device at scene load.  With HK_TREE_SAH
the mesh-level nodes must equal, byte for byte and in every ordering, those of a second context given hk_upload_scene's arrays of the
twin builder (add_mesh + hk_scene_builder_rebuild_mesh_tree), the trees written back into the builder must be the twin builder's, and
the context must be in the state an upload leaves.  Built like tests/test_mesh_rebuild_gpu.py, whose mesh generators it imports."""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from conftest import ROOT
from test_mesh_deform_gpu import SETTINGS
from test_mesh_rebuild import IDENTITY, NODE, flat, node_array
from test_mesh_rebuild_gpu import SIZED, folded_data, soup, unfold

pytestmark = pytest.mark.gpu

LEAF = 0x80000000
BUFFERS = ("vertices", "primitives", "asset_nodes", "materials", "instances", "instance_nodes", "emissives", "emissive_nodes", "alias_table")


def plugin(threaded=False, flags=0):
    if threaded:
        with product_default_traversal():
            return hk.HikariPlugin(device=0, flags=flags)
    return hk.HikariPlugin(device=0, flags=flags)


@contextlib.contextmanager
def every_mesh(how):
    """SceneBuilders used inside add every mesh deferred ('deferred') or as the twin does ('twin': add_mesh + rebuild_mesh_tree)"""
    plain = SceneBuilder.add_mesh

    def add_mesh(self, positions, normals, uvs, indices=None, topology=F.TOPOLOGY_TRIANGLE_LIST, build_tree=True):
        mesh = plain(self, positions, normals, uvs, indices, topology, build_tree=how != "deferred")
        if how == "twin":
            self.rebuild_mesh_tree(mesh)
        return mesh

    SceneBuilder.add_mesh = add_mesh
    try:
        yield
    finally:
        SceneBuilder.add_mesh = plain


def assert_builders_equal(d, t, what):
    got, want = d.scene(), t.scene()
    for n in BUFFERS:
        assert bytes(getattr(got, n)) == bytes(getattr(want, n)), f"{what}: the written-back {n} differ from the twin builder's"


def nodes_equal(gpu, twin, what):
    a, na, oa = gpu.engine.read_mesh_nodes()
    b, nb, ob = twin.engine.read_mesh_nodes()
    assert (na, oa) == (nb, ob)
    x, y = np.frombuffer(bytes(a), NODE), np.frombuffer(bytes(b), NODE)
    bad = np.flatnonzero(x.view(np.uint8).reshape(-1, 32) != y.view(np.uint8).reshape(-1, 32))
    assert bytes(a) == bytes(b), f"{what}: mesh-level nodes differ from the uploaded twin's, first at node {bad[0] // 32 if len(bad) else None} of {na} x {oa}"
    return na, oa


# ---------------------------------------------------------------------------------------------------------------- 1. sizes
def three_meshes(positions, idx, how):
    """a bystander cloth, the mesh under test, a bystander sphere: (finished builder, mesh id)"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    p, n, uv, i = S.cloth_grid(5, 4)
    ids = [b.add_mesh(p, n, uv, i)]
    n, uv = flat(positions)
    mesh = b.add_mesh(positions, n, uv, idx, build_tree=how != "deferred")
    if how == "twin":
        b.rebuild_mesh_tree(mesh)
    ids.append(mesh)
    p, n, uv, i = S._sphere(5, 6)
    ids.append(b.add_mesh(p, n, uv, i))
    for m in ids:
        b.add_instance(m, mat, IDENTITY)
    b.finish()
    return b, mesh


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("name", ["1", "2", "3", "1023", "1024", "1025", "half_split", "half_split_40000", "triplicated_42000", "130051"])
def test_loaded_mesh_equals_the_uploaded_twin(name, threaded):
    positions, _, idx = SIZED[name]
    d, mesh = three_meshes(positions, idx, "deferred")
    t, _ = three_meshes(positions, idx, "twin")
    gpu, twin, ordinary = plugin(threaded), plugin(threaded), plugin(threaded)
    assert d.pending_mesh_trees() == 1
    loaded = gpu.load_scene(d, F.TREE_SAH)
    assert d.pending_mesh_trees() == 0
    twin.set_scene(t.scene())
    count, orderings = nodes_equal(gpu, twin, name)
    assert orderings in ((1, 8) if threaded else (1,))
    assert_builders_equal(d, t, name)
    assert bytes(loaded.asset_nodes) == bytes(t.scene().asset_nodes)
    meshes, tris, launches, on_host = gpu.engine.last_load()
    assert (meshes, tris, on_host) == (1, len(idx) // 3, 0) and launches >= 4
    # the bystanders: the bytes of an ordinary upload (plain add_mesh everywhere)
    o, _ = three_meshes(positions, idx, "plain")
    ordinary.set_scene(o.scene())
    index = d.mesh_index(mesh)
    lo, hi = index.node_offset, index.node_offset + index.node_count
    got = np.frombuffer(bytes(gpu.engine.read_mesh_nodes()[0]), NODE).reshape(orderings, count)
    want = np.frombuffer(bytes(ordinary.engine.read_mesh_nodes()[0]), NODE).reshape(orderings, count)
    assert got[:, :lo].tobytes() == want[:, :lo].tobytes() and got[:, hi:].tobytes() == want[:, hi:].tobytes()
    # ... and on these inputs (no box face with both zeros) the loaded mesh too
    assert got.tobytes() == want.tobytes(), "the loaded scene differs from a plain add_mesh upload"


# ---------------------------------------------------------------------------------------------------------------- 2. forest
FOREST_SIZES = (1, 2, 3, 7, 64, 511, 1024)


def forest(how, n_small):
    """n_small deferred meshes with sizes drawn from FOREST_SIZES (fixed seed; some instanced twice, the last two never), two above
    32 768 triangles and two host-built ones: (finished builder, number of deferred meshes)"""
    rng = np.random.default_rng(20260)
    sizes = rng.choice(FOREST_SIZES, size=300)[:n_small]
    twice = rng.uniform(size=300) < 0.2
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))

    def add(positions, idx, late, instances, material=mat):
        n, uv = flat(positions)
        m = b.add_mesh(positions, n, uv, idx, build_tree=not (late and how == "deferred"))
        if late and how == "twin":
            b.rebuild_mesh_tree(m)
        for k in range(instances):
            b.add_instance(m, material, S._trs((0.1 * k, 0.05 * (m % 7), 0.0), (0.0, 0.3 * k, 0.0), (1.0, 1.0, 1.0)))

    p, _, _, i = S.cloth_grid(5, 4)
    add(p, i, False, 1)
    for k, size in enumerate(sizes):
        p, _, i = soup(int(size), 1000 + k)
        add(p, i, True, 0 if k >= n_small - 2 else (2 if twice[k] else 1), glow if k == 5 else mat)
    for size, seed in ((40000, 7), (42000, 8)):
        p, _, i = soup(size, seed)
        add(p, i, True, 1)
    p, _, _, i = S._sphere(5, 6)
    add(p, i, False, 1)
    b.finish()
    return b, n_small + 2


@pytest.mark.parametrize("threaded", [False, True])
def test_a_forest_of_meshes_is_built_at_a_launch_count_that_ignores_their_number(threaded):
    d, n_deferred = forest("deferred", 300)
    t, _ = forest("twin", 300)
    assert d.pending_mesh_trees() == n_deferred == 302
    gpu, twin, few = plugin(threaded), plugin(threaded), plugin(threaded)
    gpu.load_scene(d, F.TREE_SAH)
    twin.set_scene(t.scene())
    _, orderings = nodes_equal(gpu, twin, "forest")
    assert orderings == (8 if threaded else 1)
    assert_builders_equal(d, t, "forest")
    meshes, tris, launches, on_host = gpu.engine.last_load()
    assert (meshes, on_host) == (302, 0)
    # the same scene cut down to 3 small meshes plus the two large ones
    c, n_cut = forest("deferred", 3)
    few.load_scene(c, F.TREE_SAH)
    cut_meshes, _, cut_launches, _ = few.engine.last_load()
    assert cut_meshes == n_cut == 5
    print(f"forest: {launches} launches for {meshes} meshes / {tris} triangles, {cut_launches} for {cut_meshes} meshes")
    assert launches <= cut_launches, (launches, cut_launches)


# ---------------------------------------------------------------------------------------------------------------- 3. frames
def deferred_and_twin(make):
    with every_mesh("deferred"):
        dev = make()
    with every_mesh("twin"):
        tw = make()
    return dev, tw


def render_and_compare(plugins, cam, s, lights, frames, what):
    for n in frames:
        for p in plugins:
            p.render(cam, s, lights=lights, frame_number=n)
        base = snapshot(plugins[0])
        for k, p in enumerate(plugins[1:]):
            bad = diff_buffers(base, snapshot(p))
            assert bad == {}, f"{what}, frame {n}, against plugin {k + 1}: {bad}"


@pytest.mark.parametrize("default_traversal", [False, True])
@pytest.mark.parametrize("base", ["yard", "small"])
def test_frames_of_a_loaded_scene_equal_the_twins_and_the_oracles(base, default_traversal):
    from oracle_lib import oracle_plugin

    (dev, sun, _), (tw, _, _) = deferred_and_twin(lambda: S.deforming_scene(base))
    flags = 0 if default_traversal else F.CTX_DETERMINISTIC_SCATTER
    gpu, twin = plugin(default_traversal, flags), plugin(default_traversal, flags)
    n_pending = dev.builder.pending_mesh_trees()
    assert n_pending >= 5
    loaded = gpu.load_scene(dev.builder, F.TREE_SAH)
    assert gpu.engine.last_load()[0] == n_pending
    twin.set_scene(tw.builder.scene())
    nodes_equal(gpu, twin, base)
    assert gpu.engine.traversal_mode() == twin.engine.traversal_mode() and gpu.engine.wide_walk() == twin.engine.wide_walk()
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    plugins = [gpu, twin]
    if not default_traversal:   # (the oracle walks the reference's order: the exact contexts' frames)
        cpu = oracle_plugin()
        cpu.set_scene(loaded)   # the written-back builder
        plugins.append(cpu)
    render_and_compare(plugins, cam, s, lights, (1, 2, 3, 4), base)


def test_cornell_loaded_keeps_the_one_level_walk():
    dev, tw = deferred_and_twin(hk.load_cornell)
    with product_default_traversal():
        gpu, twin = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    gpu.load_scene(dev.builder)
    twin.set_scene(tw.builder.scene())
    assert gpu.engine.traversal_mode() == twin.engine.traversal_mode() and gpu.engine.traversal_mode()[0] == "one-level"
    nodes_equal(gpu, twin, "cornell")
    render_and_compare([gpu, twin], hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS), None, (1, 2, 3, 4), "cornell")


# ---------------------------------------------------------------------------------------------------------------- 4. state after a load
def test_the_context_is_in_the_state_an_upload_leaves():
    (dev, sun, dev_meshes), (tw, _, tw_meshes) = deferred_and_twin(lambda: S.deforming_scene("yard"))
    gpu, twin = plugin(flags=F.CTX_DETERMINISTIC_SCATTER), plugin(flags=F.CTX_DETERMINISTIC_SCATTER)
    b = dev.builder
    loaded = gpu.load_scene(b)
    twin.set_scene(tw.builder.scene())
    api, ctx = gpu.engine.api, gpu.engine.ctx
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    # an upload that lays the instance level out again from the host mirrors is taken, and the next frame renders
    assert api.raw("upload_materials")(ctx, loaded.materials, len(loaded.materials)) == F.HK_OK
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_OK
    render_and_compare([gpu, twin], cam, s, lights, (1,), "after upload_materials")
    # ray queries
    rng = np.random.default_rng(5)
    rays = hk.make_rays(rng.uniform(-3, 3, (512, 3)) + np.array([0, 6, 0]), rng.normal(size=(512, 3)) * np.array([1, 0.2, 1]) - np.array([0, 1, 0]))
    assert gpu.engine.cast_rays(rays).tobytes() == twin.engine.cast_rays(rays).tobytes()
    # a deformation finds the topology in the mirror; with a rebuild it equals the mirror sequence of the twin
    data, _ = folded_data(dev_meshes, 3)
    cl, tcl = dev_meshes["cloth"], tw_meshes["cloth"]
    gpu.engine.update_mesh_vertices(cl["index"], *data["cloth"])
    gpu.engine.rebuild_mesh_tree(cl["index"], F.TREE_SAH)
    tw.builder.set_mesh_vertices(tcl["id"], *data["cloth"])
    tw.builder.rebuild_mesh_tree(tcl["id"])
    twin.set_scene(tw.builder.finish())
    nodes_equal(gpu, twin, "deformed and rebuilt after a load")
    render_and_compare([gpu, twin], cam, s, lights, (2, 3), "after a deformation")


def test_a_second_load_builds_only_the_new_tree():
    def make(how, extra):
        with every_mesh(how):
            scene, sun, _ = S.deforming_scene("small")
        b = scene.builder
        if extra is not None:
            add_extra(b, how)
        return b, sun

    def add_extra(b, how):
        p, _, i = soup(700, 77)
        n, uv = flat(p)
        m = b.add_mesh(p, n, uv, i, build_tree=how != "deferred")
        if how == "twin":
            b.rebuild_mesh_tree(m)
        b.add_instance(m, 0, S._trs((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
        b.finish()

    d, sun = make("deferred", None)
    gpu, twin = plugin(flags=F.CTX_DETERMINISTIC_SCATTER), plugin(flags=F.CTX_DETERMINISTIC_SCATTER)
    gpu.load_scene(d)
    first = gpu.engine.last_load()
    assert first[0] >= 5 and d.pending_mesh_trees() == 0
    add_extra(d, "deferred")
    assert d.pending_mesh_trees() == 1
    gpu.load_scene(d)
    assert gpu.engine.last_load()[:2] == (1, 700) and gpu.engine.last_load()[3] == 0
    t, _ = make("twin", True)
    twin.set_scene(t.scene())
    nodes_equal(gpu, twin, "second load")
    assert_builders_equal(d, t, "second load")
    cam, lights, s = synthetic_camera(80, 56), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    render_and_compare([gpu, twin], cam, s, lights, (1, 2), "second load")
    # nothing pending: a load is an upload
    gpu.load_scene(d)
    assert gpu.engine.last_load() == (0, 0, 0, 0)
    nodes_equal(gpu, twin, "third load")


# ---------------------------------------------------------------------------------------------------------------- 5. LBVH
def test_lbvh_load_gives_valid_trees_and_frames_equal_a_twin_given_them():
    from oracle_lib import oracle_plugin

    with every_mesh("deferred"):
        dev, sun, meshes = S.deforming_scene("yard")
    b = dev.builder
    p, _, i = soup(1500, 3)   # (and one mesh above a workgroup's subtree)
    n, uv = flat(p)
    big = b.add_mesh(p, n, uv, i, build_tree=False)
    b.add_instance(big, 0, S._trs((0.0, 1.5, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    b.finish()
    gpu, twin, cpu = plugin(flags=F.CTX_DETERMINISTIC_SCATTER), plugin(flags=F.CTX_DETERMINISTIC_SCATTER), oracle_plugin()
    n_pending = b.pending_mesh_trees()
    loaded = gpu.load_scene(b, F.TREE_LBVH)
    assert gpu.engine.last_load()[0] == n_pending and b.pending_mesh_trees() == 0
    raw, count, orderings = gpu.engine.read_mesh_nodes()
    dev_nodes = np.frombuffer(bytes(raw), NODE).reshape(orderings, count)
    prims = np.frombuffer(bytes(loaded.primitives), np.dtype([("v", [("p", "<f4", 3), ("i", "<u4")], 3)]))["v"]["p"]
    host = node_array(loaded.asset_nodes)
    for mesh in [meshes["cloth"]["id"], meshes["cylinder"]["id"], meshes["sphere"]["id"], big, 0]:
        index = b.mesh_index(mesh)
        lo, hi = index.node_offset, index.node_offset + index.node_count
        n_tris = (index.node_count + 2) // 3
        a = unfold(dev_nodes[0, lo:hi])
        leaf = a["entry"] >= LEAF
        assert sorted((a["entry"][leaf] - LEAF).tolist()) == list(range(n_tris)), "every triangle exactly once"
        tris = prims[index.primitive:index.primitive + n_tris]
        tlo, thi = tris.min(axis=1), tris.max(axis=1)
        for k in np.flatnonzero(~leaf):   # every navigator: the union of the leaves of its range
            assert a["entry"][k] == k + 1 and k + 1 < a["exit"][k] <= len(a)
            shapes = (a["entry"][k + 1:a["exit"][k]][leaf[k + 1:a["exit"][k]]] - LEAF).astype(np.int64)
            assert np.array_equal(a["min"][k], tlo[shapes].min(axis=0)) and np.array_equal(a["max"][k], thi[shapes].max(axis=0)), (mesh, k)
        # the written-back tree is that tree in reference form
        a["min"][leaf], a["max"][leaf] = np.float32(np.inf), np.float32(-np.inf)
        assert host[lo:hi].tobytes() == a.tobytes(), mesh
    twin.set_scene(loaded)
    cpu.set_scene(loaded)
    nodes_equal(gpu, twin, "LBVH")
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    render_and_compare([gpu, twin, cpu], cam, s, lights, (1, 2, 3), "LBVH")


# ---------------------------------------------------------------------------------------------------------------- 6. bands
@pytest.mark.parametrize("bands,bounds", [(2, [0, 20, 64]), (3, [0, 9, 40, 64])])
def test_bands_loading_equal_the_single_context(bands, bounds):
    from bevy_hikari_amd.distributed import MultiEngine

    (dev, sun, _), (ref_scene, _, _) = deferred_and_twin(lambda: S.deforming_scene("yard"))
    s = hk.HikariSettings(**SETTINGS)
    w, h = 96, 64
    cam, lights = synthetic_camera(w, h), hk.lights_uniform(directional=sun)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    m, ref = MultiEngine([0] * bands, flags=F.CTX_DETERMINISTIC_SCATTER), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    m.upload_noise(); ref.upload_noise()
    m.load_scene(dev.builder, F.TREE_SAH)
    assert dev.builder.pending_mesh_trees() == 0
    ref.upload_scene(ref_scene.builder.scene())
    m.resize(w, h, 1.0); ref.resize(w, h, 1.0)
    m.set_band_bounds(bounds)
    want = bytes(ref.read_mesh_nodes()[0])
    for k, e in enumerate(m.contexts):
        assert bytes(e.read_mesh_nodes()[0]) == want, f"band {k}: mesh-level nodes differ from the single context's"
    for n in range(1, 4):
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        m.wait(); ref.wait()
        for b in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(b).view(np.uint8) == ref.read(b).view(np.uint8)).all(), f"{bands} bands, frame {n}: buffer {b} differs"


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing():
    positions, _, idx = SIZED["1025"]
    d, mesh = three_meshes(positions, idx, "deferred")
    t, _ = three_meshes(positions, idx, "twin")
    gpu, twin = plugin(), plugin()
    api, ctx = gpu.engine.api, gpu.engine.ctx
    # before any scene: the refusals leave the context without one
    assert api.raw("upload_scene")(ctx, d.h) == F.HK_E_NOT_READY
    assert "hk_load_scene" in api.last_error() and "hk_scene_builder_build_pending_mesh_trees" in api.last_error()
    assert api.raw("upload_scene_instances")(ctx, d.h) == F.HK_E_NOT_READY
    assert api.raw("update_scene_instances")(ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY
    mode, orderings = C.c_uint32(), C.c_uint32()
    assert api.raw("traversal_mode")(ctx, C.byref(mode), C.byref(orderings)) != F.HK_OK   # still no scene
    # with a scene: nothing of it changes
    o, _ = three_meshes(positions, idx, "plain")
    gpu.set_scene(o.scene())
    before = bytes(gpu.engine.read_mesh_nodes()[0])
    for call in ("upload_scene", "upload_scene_instances"):
        assert api.raw(call)(ctx, d.h) == F.HK_E_NOT_READY, call
    assert api.raw("update_scene_instances")(ctx, d.h, F.TREE_SAH) == F.HK_E_NOT_READY
    assert api.raw("load_scene")(ctx, d.h, 2) == F.HK_E_INVALID
    assert api.raw("load_scene")(ctx, None, F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("load_scene")(None, d.h, F.TREE_SAH) == F.HK_E_INVALID
    unfinished = SceneBuilder()
    assert api.raw("load_scene")(ctx, unfinished.h, F.TREE_SAH) == F.HK_E_NOT_READY
    assert bytes(gpu.engine.read_mesh_nodes()[0]) == before and d.pending_mesh_trees() == 1
    assert api.raw("upload_scene_instances")(ctx, o.h) == F.HK_OK   # nothing was written: no mirror is stale
    # a mesh over the device limit (the limit lowered through the debug option) is completed on the host inside the call
    gpu.engine.set_debug_option(F.DEBUG_OPT_LOAD_DEVICE_LIMIT, 1000)
    gpu.load_scene(d)
    assert gpu.engine.last_load() == (0, 0, 0, 1) and d.pending_mesh_trees() == 0
    twin.set_scene(t.scene())
    nodes_equal(gpu, twin, "host completion inside the load")
    assert_builders_equal(d, t, "host completion inside the load")
    # ... beside one the device builds
    gpu.engine.set_debug_option(F.DEBUG_OPT_LOAD_DEVICE_LIMIT, 1024)
    p, _, i = soup(1024, 9)
    for b, how in ((d, "deferred"), (t, "twin")):
        for q, qi in ((p, i), (positions * np.float32(0.5), idx)):
            n, uv = flat(q)
            m = b.add_mesh(q, n, uv, qi, build_tree=how != "deferred")
            if how == "twin":
                b.rebuild_mesh_tree(m)
            b.add_instance(m, 0, IDENTITY)
        b.finish()
    gpu.load_scene(d)
    assert gpu.engine.last_load()[:2] == (1, 1024) and gpu.engine.last_load()[3] == 1
    twin.set_scene(t.scene())
    nodes_equal(gpu, twin, "one mesh on the device, one on the host")
    assert_builders_equal(d, t, "one mesh on the device, one on the host")


# ---------------------------------------------------------------------------------------------------------------- 8. the C++ example
def test_the_cpp_example_loads_its_scene_with_device_trees(tmp_path):
    raw = tmp_path / "tm.bin"
    r = subprocess.run([os.path.join(ROOT, "examples", "cornell"), "--device-trees", "--size", "96", "64", "--frames", "3", "--bounces", "2", "--ratio", "1.0", "--raw", str(raw)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(raw, dtype=np.uint16).reshape(64, 96, 4)
    with every_mesh("deferred"):
        scene = hk.load_cornell()
    p = hk.HikariPlugin(device=0)
    p.load_scene(scene.builder)
    s = hk.HikariSettings(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
    for n in range(1, 4):
        p.render(hk.cornell_camera(96, 64), s, frame_number=n)
    assert (got == p.engine.read(F.BUF_TONE_MAPPED)).all()
