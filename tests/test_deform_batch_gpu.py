"""Many meshes deformed in one call (hk_deform_meshes).  The yardstick of every comparison is a TWIN context that makes the single-mesh
calls (hk_update_mesh_vertices / hk_skin_mesh) in item order: every screen buffer, the mesh-level nodes of every ordering, the emitter
records with the alias table and every mesh's positions, normals, triangles and box must be equal bit for bit.  Frames are 96 x 64 with
two bounces; no mesh has more than 722 triangles.

The crowd's triangle counts are the smallest at which the segmented kernels can go wrong: items that end inside a wave (2, 3, 63, 65
triangles) and inside a 256-thread workgroup (127 .. 257, 722), trees with no inner node (1 triangle) and with one (2), more items than
a wave has lanes (70) or a workgroup has threads (300), vertex updates and skins in one launch, vertex counts (triangles + 2) that are no
multiple of 64."""
import ctypes as C
import time

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import deform_items
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot

pytestmark = pytest.mark.gpu

SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
SIZES = [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 722]
CROWD = [SIZES[k % len(SIZES)] for k in range(69)] + [1]   # 70 meshes; the builder takes a mesh of one triangle
SMALL = [3, 65, 128, 257, 64]


def plugin(flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False):
    if default_traversal:
        with product_default_traversal():
            return hk.HikariPlugin(device=0, flags=flags)
    return hk.HikariPlugin(device=0, flags=flags)


def set_skins(engine, meshes):
    for m in meshes.values():
        if m["kind"] == "skin":
            engine.set_mesh_skin(m["index"], m["rest"], m["normals"], m["joints"], m["weights"])


def make_pair(base, sizes, flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False):
    """(plugin, scene, meshes) twice: the context under test and its twin, each with a scene of its own"""
    out = []
    for _ in range(2):
        scene, sun, meshes = S.crowd_scene(base, sizes)
        p = plugin(flags, default_traversal)
        p.set_scene(scene)
        set_skins(p.engine, meshes)
        out.append((p, scene, meshes))
    return out[0], out[1], sun


def single_calls(engine, items):
    """the yardstick: the parent's single-mesh calls, in item order"""
    for item in items:
        if item[0] == "skin":
            engine.skin_mesh(item[1], item[2])
        else:
            engine.update_mesh_vertices(item[1], item[2], item[3])


def assert_same_scene(a, b, meshes_a, meshes_b, what):
    """mesh-level nodes of every ordering, emitter records + alias table, every mesh's geometry"""
    na, ca, oa = a.engine.read_mesh_nodes()
    nb, cb, ob = b.engine.read_mesh_nodes()
    assert (ca, oa) == (cb, ob)
    assert bytes(na) == bytes(nb), f"{what}: mesh-level nodes differ"
    (ra, aa), (rb, ab) = a.engine.read_emitters(), b.engine.read_emitters()
    assert ra.tobytes() == rb.tobytes(), f"{what}: emitter records differ"
    assert aa.tobytes() == ab.tobytes(), f"{what}: alias tables differ"
    for name in meshes_a:
        ga, gb = a.engine.read_mesh_geometry(meshes_a[name]["index"]), b.engine.read_mesh_geometry(meshes_b[name]["index"])
        for key in ("positions", "normals", "triangles", "box"):
            assert ga[key].tobytes() == gb[key].tobytes(), f"{what}: {key} of mesh {name} differ"


def assert_same_frame(a, b, what):
    bad = diff_buffers(snapshot(a), snapshot(b))
    assert bad == {}, f"{what}: {bad}"


def frame_tools(sun, size=(96, 64), settings=SETTINGS):
    return synthetic_camera(*size), hk.lights_uniform(directional=sun), hk.HikariSettings(**settings)


def assert_same_staleness(a, scene_a, b, scene_b, what):
    """what the host may still upload, and how the scene is walked: the batch leaves the flags the single calls leave"""
    answers = []
    for p, scene in ((a, scene_a), (b, scene_b)):
        api, ctx = p.engine.api, p.engine.ctx
        mode, orderings = C.c_uint32(), C.c_uint32()
        answers.append((api.raw("upload_scene_instances")(ctx, scene.builder.h), api.raw("update_scene_instances")(ctx, scene.builder.h, F.TREE_SAH),
                        api.raw("traversal_mode")(ctx, C.byref(mode), C.byref(orderings)), mode.value, orderings.value))
    assert answers[0] == answers[1], f"{what}: {answers}"
    return answers[0]


def run_sequence(base, sizes, frames, flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False, deform_before_first=False):
    (gpu, gs, gm), (twin, ts, tm), sun = make_pair(base, sizes, flags, default_traversal)
    cam, lights, s = frame_tools(sun)
    for n in range(1, frames + 1):
        if n > 1 or deform_before_first:
            gpu.engine.deform_meshes(S.crowd_items(gm, n + 1))
            single_calls(twin.engine, S.crowd_items(tm, n + 1))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        assert_same_frame(gpu, twin, f"frame {n}")
        assert_same_scene(gpu, twin, gm, tm, f"frame {n}")
    moved = [not np.array_equal(gpu.engine.read_mesh_geometry(m["index"])["positions"], m["rest"]) for m in gm.values()]
    assert all(moved), "the poses must move every mesh: equality of two untouched scenes would show nothing"
    stale = assert_same_staleness(gpu, gs, twin, ts, "after the sequence")
    assert stale[:2] == (F.HK_E_NOT_READY, F.HK_E_NOT_READY)   # (the host mirrors no longer describe the meshes)
    return gpu, twin


# ---- 1
@pytest.mark.parametrize("default_traversal", [False, True], ids=["reference_walk", "product_default"])
def test_crowd_of_70_equals_the_single_calls(default_traversal):
    """70 meshes of 1 .. 722 triangles, half skinned (palettes of 1, 3 and 17 joints), half vertex-updated (a third without normals), two
    emissive, three instanced twice; 4 frames with a batch between them.  Once with HK_CTX_EXACT_TRAVERSAL | HK_CTX_DETERMINISTIC_SCATTER
    (the suite's flags), once with the product default: eight threaded orderings of every mesh tree and the wide records derived again."""
    assert sum(1 for k in range(len(CROWD)) if k % 2 == 0) == 35 and all((t + 2) % 64 for t in CROWD)
    gpu, _ = run_sequence("yard", CROWD, 4, flags=0 if default_traversal else F.CTX_DETERMINISTIC_SCATTER, default_traversal=default_traversal)
    d = gpu.engine.last_deform()
    assert d[:3] == (70, sum(t + 2 for t in CROWD), sum(CROWD))
    if default_traversal:
        mode, orderings = C.c_uint32(), C.c_uint32()
        gpu.engine.api.call("traversal_mode", gpu.engine.ctx, C.byref(mode), C.byref(orderings))
        assert orderings.value == 8 and mode.value & F.TRAVERSAL_WIDE


# ---- 2
def test_300_quads_in_one_batch():
    """More items than a workgroup has threads, two triangles (one inner node) each: one batch, one frame."""
    run_sequence("yard", [2] * 300, 1, deform_before_first=True)


# ---- 3
def test_small_scene_from_the_lds_copy():
    """The small base (it fits the LDS copy) with 5 meshes, 3 frames."""
    run_sequence("small", SMALL, 3)


# ---- 4
def test_crowd_frame_equals_the_uploaded_builder_mirror():
    """One frame of the crowd against the host's own path: a context given the builder-mirrored scene (set_mesh_vertices + finish + upload),
    as test_mesh_deform_gpu.py does for single calls.  Skinned meshes are mirrored through scenes.skin_reference."""
    scene, sun, meshes = S.crowd_scene("yard", CROWD)
    mirror_scene, _, mirror_meshes = S.crowd_scene("yard", CROWD)
    gpu, twin = plugin(), plugin()
    gpu.set_scene(scene)
    twin.set_scene(mirror_scene)
    set_skins(gpu.engine, meshes)
    cam, lights, s = frame_tools(sun)
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)
    assert_same_frame(gpu, twin, "frame 1")
    gpu.engine.deform_meshes(S.crowd_items(meshes, 3))
    b = mirror_scene.builder
    for m in mirror_meshes.values():
        if m["kind"] == "skin":
            q, qn = S.skin_reference(m["rest"], m["normals"], m["joints"], m["weights"], m["pose"](3)[0])
        else:
            q, qn = m["pose"](3)
        b.set_mesh_vertices(m["id"], q, qn)
    twin.set_scene(b.finish())
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=2)
    assert_same_frame(gpu, twin, "frame 2")
    na, ca, oa = gpu.engine.read_mesh_nodes()
    nb, cb, ob = twin.engine.read_mesh_nodes()
    assert (ca, oa) == (cb, ob) and bytes(na) == bytes(nb), "mesh-level nodes differ from the uploaded mirror's"


# ---- 5
def test_launch_counts_do_not_depend_on_the_number_of_items():
    """A batch of 3 and a batch of 70 enqueue the same number of launches, and so do the flush and the wide-record derivation of the
    frame that follows - also after 70 single calls.  Each stays below 16: the design needs 5 (begin, vertices, triangles, boxes, emit),
    4 (instances, emitters, instance tree, light tree) and 2 (mesh trees, instance tree)."""
    scene, sun, meshes = S.crowd_scene("yard", CROWD)
    p = plugin(flags=0, default_traversal=True)
    p.set_scene(scene)
    set_skins(p.engine, meshes)
    cam, lights, s = frame_tools(sun)
    p.render(cam, s, lights=lights, frame_number=1)
    items = S.crowd_items(meshes, 2)
    emissive = [k for k, inst in enumerate(scene.instances) if any(e.instance == k for e in scene.emissives)]
    glowing = [k for k, m in enumerate(meshes.values()) if any(bytes(scene.instances[i].mesh) == bytes(m["index"]) for i in emissive)]
    assert len(glowing) == 2
    three = [items[glowing[0]], items[0], items[5]]
    counts = []
    for n, batch in ((2, three), (3, items)):
        p.engine.deform_meshes(batch)
        p.render(cam, s, lights=lights, frame_number=n)
        counts.append(p.engine.last_deform())
    assert counts[0][0] == 3 and counts[1][0] == 70
    assert counts[0][3:] == counts[1][3:], counts
    assert all(0 < c < 16 for c in counts[1][3:]), counts
    single_calls(p.engine, S.crowd_items(meshes, 4))
    p.render(cam, s, lights=lights, frame_number=4)
    after_single = p.engine.last_deform()
    assert after_single[4:] == counts[1][4:], (after_single, counts)
    p.engine.wait()


# ---- 6
def test_refused_batches_write_nothing():
    """A batch of 10 with one bad item at position 6, for every error kind and for a mesh named twice: the error is returned, hk_last_error
    names item 6, and the next frame and the geometry of all ten meshes equal a twin that made no call at all."""
    (gpu, gs, gm), (twin, _, tm), sun = make_pair("yard", CROWD[:12])   # meshes 10 (17 joints) and 11 (vertex-updated) stay outside the batch
    api, ctx = gpu.engine.api, gpu.engine.ctx
    names = list(gm)
    good = S.crowd_items(gm, 2)[:10]
    assert good[6][0] == "skin" and good[5][0] == "vertices"
    m6, m10, m11 = (gm[names[k]] for k in (6, 10, 11))
    assert m10["kind"] == "skin" and int(m10["joints"].max()) == 16 and m11["kind"] == "vertices"
    identity = lambda n: np.tile(np.eye(4, dtype=np.float32).reshape(-1), (n, 1))
    unknown = F.HkMeshIndex(m6["index"].vertex, m6["index"].primitive, m6["index"].node_offset + 1, m6["index"].node_count)
    swap = lambda item: good[:6] + [item] + good[7:]
    cases = {
        "unknown mesh record": (swap(("vertices", unknown, m6["rest"], None)), None),
        "too many vertices": (swap(("vertices", m11["index"], np.zeros((len(m11["rest"]) + 7, 3), np.float32), None)), None),
        "too few vertices": (swap(("vertices", m11["index"], np.zeros((2, 3), np.float32), None)), None),
        "no skin set": (swap(("skin", m11["index"], identity(3))), None),
        "a joint index at or above count": (swap(("skin", m10["index"], identity(3))), None),
        "NULL data": (good, lambda t: setattr(t[6], "data", None)),
        "normals on a skin item": (good, lambda t: setattr(t[6], "normals", t[5].data)),
        "unknown kind": (good, lambda t: setattr(t[6], "kind", 7)),
        "a mesh named twice": (swap(good[2]), None),
    }
    for what, (items, patch) in cases.items():
        assert len(items) == 10
        table, keep = deform_items(items)
        if patch:
            patch(table)
        rc = api.raw("deform_meshes")(ctx, table, len(items))
        message = api.last_error()
        assert rc == F.HK_E_INVALID, (what, rc, message)
        assert "item 6" in message, (what, message)
    assert api.raw("deform_meshes")(ctx, None, 0) == F.HK_OK   # n == 0: nothing to do
    assert gpu.engine.last_deform()[:4] == (0, 0, 0, 0)
    cam, lights, s = frame_tools(sun)
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)
    assert_same_frame(gpu, twin, "after the refusals")
    assert_same_scene(gpu, twin, {k: gm[k] for k in names[:10]}, {k: tm[k] for k in names[:10]}, "after the refusals")
    # nothing was deformed: the host mirrors still describe the device scene (a deformation makes this call return HK_E_NOT_READY)
    assert api.raw("upload_scene_instances")(ctx, gs.builder.h) == F.HK_OK


# ---- 7
def test_batch_composes_with_single_calls_refits_and_rebuilds():
    (gpu, gs, gm), (twin, ts, tm), sun = make_pair("yard", CROWD[:24])
    cam, lights, s = frame_tools(sun)
    names = list(gm)
    other = names[8]   # a skinned mesh left out of the batch
    assert gm[other]["kind"] == "skin"
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)

    def step(n, what, act):
        act(gpu, gs, gm, True)
        act(twin, ts, tm, False)
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        assert_same_frame(gpu, twin, what)
        assert_same_scene(gpu, twin, gm, tm, what)

    movers = (3, len(gs.instances) - 2)
    rest = {i: np.ctypeslib.as_array(gs.instances[i].model).copy() for i in movers}

    def batch_single_refit(p, scene, meshes, batched):
        items = [it for k, it in zip(meshes, S.crowd_items(meshes, 2)) if k != other]
        (p.engine.deform_meshes if batched else lambda its: single_calls(p.engine, its))(items)
        p.engine.skin_mesh(meshes[other]["index"], *meshes[other]["pose"](2))
        for i in movers:
            moved = rest[i].copy()
            moved[12] += 0.2
            scene.builder.set_instance_transform(i, moved)
        assert p.engine.refit_instances(scene.builder) == 2

    def rebuild_then_batch(p, scene, meshes, batched):
        p.engine.rebuild_mesh_tree(meshes[names[11]]["index"], F.TREE_SAH)   # 722 triangles: the refit climbs the new topology
        items = S.crowd_items(meshes, 3)
        (p.engine.deform_meshes if batched else lambda its: single_calls(p.engine, its))(items)

    def two_batches(p, scene, meshes, batched):
        for n in (4, 5):
            items = S.crowd_items(meshes, n)
            if n == 5:
                items = items[::-1][:13]   # another order, another subset
            (p.engine.deform_meshes if batched else lambda its: single_calls(p.engine, its))(items)

    step(2, "batch + single skin + instance refit", batch_single_refit)
    step(3, "mesh tree rebuild + batch", rebuild_then_batch)
    step(4, "two batches, no frame between", two_batches)


# ---- 8
def test_frames_in_flight_see_their_own_meshes():
    """Frame n, the batch, frame n + 1, frame n + 2 enqueued without a wait equal the twin's single calls with a wait after every frame."""
    (gpu, _, gm), (twin, _, tm), sun = make_pair("yard", CROWD)
    cam, lights, s = frame_tools(sun)
    gpu.render(cam, s, lights=lights, frame_number=1)
    gpu.engine.deform_meshes(S.crowd_items(gm, 2))
    gpu.render(cam, s, lights=lights, frame_number=2)
    gpu.render(cam, s, lights=lights, frame_number=3)
    twin.render(cam, s, lights=lights, frame_number=1)
    twin.engine.wait()
    single_calls(twin.engine, S.crowd_items(tm, 2))
    for n in (2, 3):
        twin.render(cam, s, lights=lights, frame_number=n)
        twin.engine.wait()
    assert_same_frame(gpu, twin, "three frames in flight")
    assert_same_scene(gpu, twin, gm, tm, "three frames in flight")


# ---- 9
def test_a_warm_batch_never_waits_for_the_device():
    """The criterion of test_many_deformations_between_frames_never_wait_for_the_device: with a long frame (1080p, 8 bounces) running, the
    batch of 70 returns in under half that frame's time after one warm round - it only enqueues."""
    scene, sun, meshes = S.crowd_scene("yard", CROWD)
    p = plugin()
    p.set_scene(scene)
    set_skins(p.engine, meshes)
    cam, lights = synthetic_camera(1920, 1080), hk.lights_uniform(directional=sun)
    s = hk.HikariSettings(indirect_bounces=8, upscale=hk.Upscale.SMAA_TU_1_0)
    p.render(cam, s, lights=lights, frame_number=1)
    p.engine.wait()
    t0 = time.perf_counter()
    p.render(cam, s, lights=lights, frame_number=2)
    p.engine.wait()
    frame_s = time.perf_counter() - t0
    table, keep = deform_items(S.crowd_items(meshes, 3))
    for warm in range(2):   # (the first round creates the meshes' refit planes and the staging block)
        p.render(cam, s, lights=lights, frame_number=3 + warm)
        t0 = time.perf_counter()
        p.engine.api.call("deform_meshes", p.engine.ctx, table, 70)
        call_s = time.perf_counter() - t0
        p.engine.wait()
    print(f"batch of 70: {call_s * 1e3:.3f} ms beside a frame of {frame_s * 1e3:.3f} ms")
    assert call_s < 0.5 * frame_s, (call_s, frame_s)


# ---- 10
@pytest.mark.parametrize("bands,bounds", [(2, [0, 20, 64]), (3, [0, 9, 40, 64])])
def test_bands_take_the_batch_like_the_single_context(bands, bounds):
    from bevy_hikari_amd.distributed import MultiEngine

    scene, sun, meshes = S.crowd_scene("small", SMALL)
    s = hk.HikariSettings(**SETTINGS)
    w, h = 96, 64
    cam, lights = synthetic_camera(w, h), hk.lights_uniform(directional=sun)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    m, ref = MultiEngine([0] * bands, flags=F.CTX_DETERMINISTIC_SCATTER), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    for t in (m, ref):
        t.upload_noise(); t.upload_scene(scene); t.resize(w, h, 1.0)
    m.set_band_bounds(bounds)
    for t in (m, ref):
        set_skins(t, meshes)
    for n in range(1, 4):
        if n > 1:
            m.deform_meshes(S.crowd_items(meshes, n))
            single_calls(ref, S.crowd_items(meshes, n))
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        m.wait(); ref.wait()
        for b in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(b).view(np.uint8) == ref.read(b).view(np.uint8)).all(), f"{bands} bands, frame {n}: buffer {b} differs"
    geo = ref.read_mesh_geometry(meshes["m3"]["index"])
    for band_geo in m.read_mesh_geometry(meshes["m3"]["index"]):
        for key in ("positions", "normals", "triangles", "box"):
            assert band_geo[key].tobytes() == geo[key].tobytes(), f"{bands} bands: {key} differ"
