"""Mesh deformation on the device (hk_update_mesh_vertices, hk_set_mesh_skin + hk_skin_mesh): every frame of a deforming sequence must
equal, bit for bit, a second context given the builder-mirrored scene (hk_scene_builder_set_mesh_vertices + hk_upload_scene) - the
host's own path - and the mesh-level nodes of every ordering must be the ones that upload lays out.  Traversals: the reference walk of
the suite (HK_CTX_EXACT_TRAVERSAL) and the product default beyond the LDS copy (threaded orderings + wide records, wavefront schedule)."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot

pytestmark = pytest.mark.gpu

SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)


def frame_data(meshes, frame):
    """(positions, normals) of every deforming mesh at `frame`, and the cylinder's joints"""
    cl, sp, cy = meshes["cloth"], meshes["sphere"], meshes["cylinder"]
    out = {"cloth": S.waving_cloth(cl["rest"], frame, amplitude=0.15), "sphere": (S.pulsing_sphere(sp["rest"], frame), None)}
    joints = S.bend_joints(frame)
    out["cylinder"] = S.skin_reference(cy["rest"], cy["normals"], cy["joints"], cy["weights"], joints)
    return out, joints


def deform_device(engine, meshes, data, joints, skinned=True):
    engine.update_mesh_vertices(meshes["cloth"]["index"], *data["cloth"])
    engine.update_mesh_vertices(meshes["sphere"]["index"], data["sphere"][0])
    if skinned:
        engine.skin_mesh(meshes["cylinder"]["index"], joints)
    else:
        engine.update_mesh_vertices(meshes["cylinder"]["index"], *data["cylinder"])


def mirror(builder, meshes, data):
    for name, (p, n) in data.items():
        builder.set_mesh_vertices(meshes[name]["id"], p, n)
    scene = builder.finish()
    return scene


def make_pair(base, flags=0, default_traversal=False):
    def plugin():
        if default_traversal:
            with product_default_traversal():
                return hk.HikariPlugin(device=0, flags=flags)
        return hk.HikariPlugin(device=0, flags=flags)

    dev_scene, sun, dev_meshes = S.deforming_scene(base)
    twin_scene, _, twin_meshes = S.deforming_scene(base)
    gpu, twin = plugin(), plugin()
    gpu.set_scene(dev_scene)
    twin.set_scene(twin_scene)
    cy = dev_meshes["cylinder"]
    gpu.engine.set_mesh_skin(cy["index"], cy["rest"], cy["normals"], cy["joints"], cy["weights"])
    return gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun


def run_sequence(base, frames=8, flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False, size=(96, 64), compare_nodes=True, expect_mode=None):
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair(base, flags, default_traversal)
    cam = synthetic_camera(*size)
    lights = hk.lights_uniform(directional=sun)
    s = hk.HikariSettings(**SETTINGS)
    for n in range(1, frames + 1):
        if n > 1:
            data, joints = frame_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            twin.set_scene(mirror(twin_scene.builder, twin_meshes, data))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"
        if compare_nodes:
            a, na, oa = gpu.engine.read_mesh_nodes()
            b, nb, ob = twin.engine.read_mesh_nodes()
            assert (na, oa) == (nb, ob)
            assert bytes(a) == bytes(b), f"frame {n}: mesh-level nodes differ from the uploaded mirror's"
    if expect_mode is not None:
        mode, orderings = C.c_uint32(), C.c_uint32()
        gpu.engine.api.call("traversal_mode", gpu.engine.ctx, C.byref(mode), C.byref(orderings))
        assert mode.value & 0xFF == expect_mode
    return gpu, twin


def test_deform_sequence_reference_walk_equals_uploaded_mirror():
    """HK_CTX_EXACT_TRAVERSAL (the suite's flags): cloth (host update), skinned cylinder, pulsing emissive sphere, 8 frames."""
    run_sequence("yard", expect_mode=0)   # HK_TRAVERSAL_REFERENCE


def test_deform_sequence_product_default_threaded_wide():
    """Beyond the LDS copy with the product's flags: eight direction-threaded orderings of every mesh tree (the device re-threads the
    refit tree by hk_bvh_rethread's rule), the wide records derived again, the wavefront schedule."""
    run_sequence("yard", flags=0, default_traversal=True)


def test_deform_sequence_small_scene():
    """The small yard: fewer instances, the same three deforming meshes."""
    run_sequence("small", size=(80, 56))


def test_emitter_records_and_light_tree_follow_the_pulsing_sphere():
    gpu, twin = run_sequence("yard", frames=4, compare_nodes=False)
    tw = twin.engine
    # the twin's light tree was BUILT for the new boxes, the device's refit: compare the emitter records through the trees' leaves
    n_t, n_l = len(S.deforming_scene("yard")[0].instance_nodes), len(S.deforming_scene("yard")[0].emissive_nodes)
    _, la = gpu.engine.read_trees(n_t, n_l)
    _, lb = tw.read_trees(n_t, n_l)
    leaves = lambda t: sorted((n.entry_index, tuple(n.min), tuple(n.max)) for n in t if n.entry_index >= 0x80000000)
    assert leaves(la) == leaves(lb)


@pytest.mark.parametrize("calls", ["single", "batch"])
@pytest.mark.parametrize("default_traversal", [False, True], ids=["reference_walk", "product_default"])
def test_deformations_at_the_edges_of_a_wave_and_a_workgroup(default_traversal, calls):
    """The vertex counts at which the wave-wide box reduction and the workgroup tables can go wrong (the crowds of test_deform_batch_gpu.py
    avoid every multiple of 64): 3 (a tree of one leaf), 4 (one inner node), 64 (exactly one wave), 256 (exactly one workgroup), 257 (one
    vertex into a second workgroup).  Every mesh through hk_update_mesh_vertices with normals, then without, then the skinned ones through
    hk_skin_mesh - or each round as one hk_deform_meshes batch; after each round the mesh nodes of every ordering and every mesh's geometry
    equal the uploaded builder mirror's, and so does one frame."""
    sizes = [1, 2, 62, 254, 255]
    (scene, sun, meshes), (twin_scene, _, twin_meshes) = S.crowd_scene("small", sizes), S.crowd_scene("small", sizes)
    assert [len(m["rest"]) for m in meshes.values()] == [3, 4, 64, 256, 257]
    assert [m["kind"] for m in meshes.values()] == ["skin", "vertices", "skin", "vertices", "skin"]
    if default_traversal:
        with product_default_traversal():
            gpu, twin = hk.HikariPlugin(device=0, flags=0), hk.HikariPlugin(device=0, flags=0)
    else:
        gpu, twin = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER), hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    gpu.set_scene(scene)
    twin.set_scene(twin_scene)
    for m in meshes.values():
        if m["kind"] == "skin":
            gpu.engine.set_mesh_skin(m["index"], m["rest"], m["normals"], m["joints"], m["weights"])

    def same_scene(what):
        a, na, oa = gpu.engine.read_mesh_nodes()
        b, nb, ob = twin.engine.read_mesh_nodes()
        assert (na, oa) == (nb, ob) and oa == (8 if default_traversal else 1)
        assert bytes(a) == bytes(b), f"{what}: mesh-level nodes differ from the uploaded mirror's"
        for name, m in meshes.items():
            g, w = gpu.engine.read_mesh_geometry(m["index"]), twin.engine.read_mesh_geometry(twin_meshes[name]["index"])
            for key in ("positions", "normals", "triangles", "box"):
                assert g[key].tobytes() == w[key].tobytes(), f"{what}: {key} of mesh {name} ({len(m['rest'])} vertices) differ from the mirror's"

    rounds = (("with normals", 2, lambda q, qn: (q, qn)), ("without normals", 3, lambda q, qn: (q, None)))
    def deform(items):
        if calls == "batch":
            return gpu.engine.deform_meshes(items)
        for kind, *args in items:
            (gpu.engine.skin_mesh if kind == "skin" else gpu.engine.update_mesh_vertices)(*args)

    for what, frame, take in rounds:
        items = []
        for name, m in meshes.items():
            data = take(*S.swaying_ribbon(m["rest"], m["normals"], frame, 0.37 * len(m["rest"])))
            items.append(("vertices", m["index"]) + data)
            twin_scene.builder.set_mesh_vertices(twin_meshes[name]["id"], *data)
        deform(items)
        twin.set_scene(twin_scene.builder.finish())
        same_scene(f"vertex updates {what}")
    items = []
    for name, m in meshes.items():
        if m["kind"] == "skin":
            joints = m["pose"](4)[0]
            items.append(("skin", m["index"], joints))
            twin_scene.builder.set_mesh_vertices(twin_meshes[name]["id"], *S.skin_reference(m["rest"], m["normals"], m["joints"], m["weights"], joints))
    deform(items)
    twin.set_scene(twin_scene.builder.finish())
    same_scene("skins")
    cam, lights, s = synthetic_camera(64, 48), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad


@pytest.mark.parametrize("deform_first", [True, False])
def test_instance_motion_and_deformation_compose(deform_first):
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    cloth_instance = len(dev_scene.instances) - 3
    rest = np.ctypeslib.as_array(dev_scene.instances[cloth_instance].model).copy()
    for n in range(1, 5):
        if n > 1:
            data, joints = frame_data(dev_meshes, n)
            moved = rest.copy()
            moved[12] += 0.1 * n
            dev_scene.builder.set_instance_transform(cloth_instance, moved)
            twin_scene.builder.set_instance_transform(cloth_instance, moved)
            if deform_first:
                deform_device(gpu.engine, dev_meshes, data, joints)
                assert gpu.engine.refit_instances(dev_scene.builder) == 1
            else:
                assert gpu.engine.refit_instances(dev_scene.builder) == 1
                deform_device(gpu.engine, dev_meshes, data, joints)
            twin.set_scene(mirror(twin_scene.builder, twin_meshes, data))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"


def test_frames_in_flight_see_their_own_mesh():
    """Three frames enqueued without a read, deformations between them, equal the same frames rendered one at a time."""
    runs = []
    for wait in (False, True):
        scene, sun, meshes = S.deforming_scene("yard")
        p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
        p.set_scene(scene)
        cy = meshes["cylinder"]
        p.engine.set_mesh_skin(cy["index"], cy["rest"], cy["normals"], cy["joints"], cy["weights"])
        cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
        for n in range(1, 4):
            if n > 1:
                data, joints = frame_data(meshes, n)
                deform_device(p.engine, meshes, data, joints)
            p.render(cam, s, lights=lights, frame_number=n)
            if wait:
                p.engine.wait()
        runs.append(snapshot(p))
    assert diff_buffers(runs[0], runs[1]) == {}


def test_stale_host_mirrors_are_refused():
    scene, sun, meshes = S.deforming_scene("yard")
    p = hk.HikariPlugin(device=0)
    p.set_scene(scene)
    api, ctx = p.engine.api, p.engine.ctx
    cam, lights, s = synthetic_camera(64, 48), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    p.render(cam, s, lights=lights, frame_number=1)
    data, _ = frame_data(meshes, 3)
    p.engine.update_mesh_vertices(meshes["cloth"]["index"], *data["cloth"])
    b = scene.builder
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_E_NOT_READY
    assert api.raw("update_scene_instances")(ctx, b.h, F.TREE_SAH) == F.HK_E_NOT_READY
    assert api.raw("rebuild_scene_trees")(ctx, F.TREE_SAH) == F.HK_OK   # works from the device's current boxes
    p.render(cam, s, lights=lights, frame_number=2)
    # materials / textures are taken, and the next use of the scene refuses to lay it out from the stale mirrors
    mode, orderings = C.c_uint32(), C.c_uint32()
    assert api.raw("upload_materials")(ctx, scene.materials, len(scene.materials)) == F.HK_OK
    assert api.raw("traversal_mode")(ctx, C.byref(mode), C.byref(orderings)) == F.HK_E_NOT_READY
    # the mirror brings the host's version back: everything is allowed again
    b.set_mesh_vertices(meshes["cloth"]["id"], *data["cloth"])
    p.set_scene(b.finish())
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_OK
    p.render(cam, s, lights=lights, frame_number=3)


def test_argument_errors_write_nothing():
    scene, sun, meshes = S.deforming_scene("yard")
    p = hk.HikariPlugin(device=0)
    p.set_scene(scene)
    api, ctx = p.engine.api, p.engine.ctx
    cl = meshes["cloth"]
    pos = np.ascontiguousarray(cl["rest"], np.float32)
    fp = pos.ctypes.data_as(C.POINTER(F.f32))
    bad = F.HkMeshIndex(cl["index"].vertex, cl["index"].primitive, cl["index"].node_offset + 1, cl["index"].node_count)
    assert api.raw("update_mesh_vertices")(ctx, C.byref(bad), len(pos), fp, None) == F.HK_E_INVALID
    assert api.raw("update_mesh_vertices")(ctx, C.byref(cl["index"]), len(pos) + 1000, fp, None) == F.HK_E_INVALID
    assert api.raw("update_mesh_vertices")(ctx, C.byref(cl["index"]), 3, fp, None) == F.HK_E_INVALID
    j = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (3, 1))
    assert api.raw("skin_mesh")(ctx, C.byref(meshes["cylinder"]["index"]), j.ctypes.data_as(C.POINTER(F.f32)), 3) == F.HK_E_INVALID  # no skin yet
    cy = meshes["cylinder"]
    p.engine.set_mesh_skin(cy["index"], cy["rest"], cy["normals"], cy["joints"], cy["weights"])
    assert api.raw("skin_mesh")(ctx, C.byref(cy["index"]), j.ctypes.data_as(C.POINTER(F.f32)), 2) == F.HK_E_INVALID  # joint 2 named
    # nothing was written: the scene still uploads instances (no deformation happened)
    assert api.raw("upload_scene_instances")(ctx, scene.builder.h) == F.HK_OK


def test_emitter_records_and_alias_table_equal_the_mirror():
    """The pulsing emissive sphere: every emitter record (position, radius, surface area, alias slice) and the whole alias table equal
    the uploaded mirror's, bit for bit, frame after frame."""
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    for n in range(2, 6):
        data, joints = frame_data(dev_meshes, n)
        deform_device(gpu.engine, dev_meshes, data, joints)
        twin.set_scene(mirror(twin_scene.builder, twin_meshes, data))
        (ra, aa), (rb, ab) = gpu.engine.read_emitters(), twin.engine.read_emitters()
        assert ra.tobytes() == rb.tobytes(), f"frame {n}: emitter records differ"
        assert aa.tobytes() == ab.tobytes(), f"frame {n}: alias tables differ"


def test_deform_sequence_vs_oracle():
    """The oracle fed the mirrored arrays (SceneData) on the device's tree shapes - the instance and light trees are refit, not rebuilt,
    so they get the device's links with every box re-derived - agrees with every buffer of every frame."""
    from oracle_lib import oracle_plugin
    from test_device_refit import refit_nodes

    gpu, _, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cpu = oracle_plugin()
    cpu.set_scene(twin_scene)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for n in range(1, 5):
        if n > 1:
            data, joints = frame_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            new = mirror(twin_scene.builder, twin_meshes, data)
            topo_t, topo_l = gpu.engine.read_trees(len(new.instance_nodes), len(new.emissive_nodes))
            boxes = np.array([[list(i.min), list(i.max)] for i in new.instances], dtype=np.float32)
            eboxes = np.array([[[e.position[k] - e.radius for k in range(3)], [e.position[k] + e.radius for k in range(3)]] for e in new.emissives], dtype=np.float32)
            expected = hk.SceneData(previous_transforms=new.previous_transforms, vertices=new.vertices, primitives=new.primitives, asset_nodes=new.asset_nodes,
                                    materials=new.materials, instances=new.instances, instance_nodes=refit_nodes(topo_t, boxes), emissives=new.emissives,
                                    emissive_nodes=refit_nodes(topo_l, eboxes), alias_table=new.alias_table)
            cpu.set_scene(expected)
        for p in (gpu, cpu):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(cpu))
        assert bad == {}, f"frame {n}: {bad}"


@pytest.mark.parametrize("bands,bounds", [(2, [0, 20, 64]), (3, [0, 9, 40, 64])])
def test_bands_deforming_equal_the_single_context(bands, bounds):
    from bevy_hikari_amd.distributed import MultiEngine

    scene, sun, meshes = S.deforming_scene("yard")
    s = hk.HikariSettings(**SETTINGS)
    w, h = 96, 64
    cam, lights = synthetic_camera(w, h), hk.lights_uniform(directional=sun)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    m, ref = MultiEngine([0] * bands, flags=F.CTX_DETERMINISTIC_SCATTER), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    for t in (m, ref):
        t.upload_noise(); t.upload_scene(scene); t.resize(w, h, 1.0)
    m.set_band_bounds(bounds)
    cy = meshes["cylinder"]
    for t in (m, ref):
        t.set_mesh_skin(cy["index"], cy["rest"], cy["normals"], cy["joints"], cy["weights"])
    for n in range(1, 5):
        if n > 1:
            data, joints = frame_data(meshes, n)
            for t in (m, ref):
                deform_device(t, meshes, data, joints)
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        m.wait(); ref.wait()
        for b in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(b).view(np.uint8) == ref.read(b).view(np.uint8)).all(), f"{bands} bands, frame {n}: buffer {b} differs"


def test_cloth_in_the_cornell_box_leaves_the_one_level_walk_until_the_mirror_is_uploaded():
    """The Cornell box walks its one-level tree (instances under one transform, LDS copy).  A cloth deformed on the device is not in
    that tree: the scene walks its two-level trees from the deformation on (hk_traversal_mode says so) - frames equal to the uploaded
    mirror walked the same way - and the one-level walk returns with the upload of the mirror."""
    def cornell_cloth():
        scene = hk.load_cornell()
        b = scene.builder
        p, n, uv, idx = S.cloth_grid(3, 3, size=1.0)   # (small: the scene has to stay inside the LDS copy with its one-level tree)
        p = p + np.array([0.0, 1.0, 0.0], np.float32)
        mid = b.add_mesh(p, n, uv, idx)
        b.add_instance(mid, 0, np.ctypeslib.as_array(scene.instances[0].model).copy())
        scene = b.finish()
        scene.builder = b
        return scene, mid, b.mesh_index(mid), p

    with product_default_traversal():
        gpu, twin = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    (dev, mid, index, rest), (tw, tmid, _, _) = cornell_cloth(), cornell_cloth()
    gpu.set_scene(dev)
    twin.set_scene(tw)
    twin.engine.api.call("debug_set_option", twin.engine.ctx, F.DEBUG_OPT_FLAT_WALK, 0)   # the twin walks two levels as the deformed scene does
    cam, s = hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS)

    def mode(p):
        m, o = C.c_uint32(), C.c_uint32()
        p.engine.api.call("traversal_mode", p.engine.ctx, C.byref(m), C.byref(o))
        return m.value & 0xFF

    assert mode(gpu) == 2   # HK_TRAVERSAL_ONE_LEVEL
    for n in range(1, 5):
        if n > 1:
            q, qn = S.waving_cloth(rest - np.array([0.0, 1.0, 0.0], np.float32), n, amplitude=0.1)
            q = q + np.array([0.0, 1.0, 0.0], np.float32)
            gpu.engine.update_mesh_vertices(index, q, qn)
            assert mode(gpu) == 0   # HK_TRAVERSAL_REFERENCE
            tw.builder.set_mesh_vertices(tmid, q, qn)
            twin.set_scene(tw.builder.finish())
        for p in (gpu, twin):
            p.render(cam, s, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"
    dev.builder.set_mesh_vertices(mid, q, qn)
    gpu.set_scene(dev.builder.finish())
    assert mode(gpu) == 2


def test_many_deformations_between_frames_never_wait_for_the_device():
    """Deformation calls between two frames only enqueue: with a long frame still running on the device, ten calls return long before
    it ends (a call that waited for an earlier one's kernels - which sit behind that frame - would take the frame's time)."""
    scene, sun, meshes = S.deforming_scene("yard")
    p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    p.set_scene(scene)
    cam, lights = synthetic_camera(1920, 1080), hk.lights_uniform(directional=sun)
    s = hk.HikariSettings(indirect_bounces=8, upscale=hk.Upscale.SMAA_TU_1_0)
    p.render(cam, s, lights=lights, frame_number=1)
    p.engine.wait()
    import time

    t0 = time.perf_counter()
    p.render(cam, s, lights=lights, frame_number=2)
    p.engine.wait()
    frame_s = time.perf_counter() - t0
    data, _ = frame_data(meshes, 3)
    for warm in range(2):   # (the first round may allocate staging buffers)
        p.render(cam, s, lights=lights, frame_number=3 + warm)
        t0 = time.perf_counter()
        for k in range(10):
            p.engine.update_mesh_vertices(meshes["cloth"]["index"], *data["cloth"])
        calls_s = time.perf_counter() - t0
        p.engine.wait()
    assert calls_s < 0.5 * frame_s, (calls_s, frame_s)
