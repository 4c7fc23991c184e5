"""hk_rebuild_mesh_tree: a deformed mesh's tree rebuilt on the device.  With HK_TREE_SAH the mesh-level nodes must equal, byte for byte
and in every ordering, those of a second context given the builder's mirror (hk_scene_builder_set_mesh_vertices +
hk_scene_builder_rebuild_mesh_tree + hk_upload_scene), the links a fresh hk_scene_builder_add_mesh over the same positions gives, and
every buffer of every frame the twin's.  Built like tests/test_mesh_deform_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from test_mesh_deform import big_mesh, big_mesh_frame
from test_mesh_deform_gpu import SETTINGS, deform_device, frame_data, make_pair
from test_mesh_rebuild import IDENTITY, NODE, flat, half_split_mesh, node_array

pytestmark = pytest.mark.gpu

LEAF = 0x80000000
NAMES = ("cloth", "sphere", "cylinder")


def folded_data(meshes, frame):
    """frame_data with the cloth folded onto itself instead of waving (half way at even frames, all the way at odd ones)"""
    data, joints = frame_data(meshes, frame)
    data["cloth"] = S.folded_cloth(meshes["cloth"]["rest"], fold=1.0 if frame % 2 else 0.5, gap=0.05)
    return data, joints


def mirror(builder, meshes, data, rebuild=()):
    for name, (p, n) in data.items():
        builder.set_mesh_vertices(meshes[name]["id"], p, n)
    for name in rebuild:
        builder.rebuild_mesh_tree(meshes[name]["id"])
    return builder.finish()


def nodes_equal(gpu, twin, what):
    a, na, oa = gpu.engine.read_mesh_nodes()
    b, nb, ob = twin.engine.read_mesh_nodes()
    assert (na, oa) == (nb, ob)
    assert bytes(a) == bytes(b), f"{what}: mesh-level nodes differ from the uploaded mirror's"


def run_sequence(base, flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False, size=(96, 64), frames=6, other=None):
    """frames 2, 4: deform (fold; the cylinder skinned) and rebuild every deforming mesh; frames 3, 5, ..: deform alone - a refit of the
    NEW shape.  `other`: a plugin fed the mirror too (the oracle)."""
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair(base, flags, default_traversal)
    cam, lights, s = synthetic_camera(*size), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for n in range(1, frames + 1):
        if n > 1:
            data, joints = folded_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            rebuild = NAMES if n in (2, 4) else ()
            for name in rebuild:
                gpu.engine.rebuild_mesh_tree(dev_meshes[name]["index"], F.TREE_SAH)
            twin.set_scene(mirror(twin_scene.builder, twin_meshes, data, rebuild))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"
        nodes_equal(gpu, twin, f"frame {n}")
    return gpu, twin


def test_rebuild_sequence_reference_walk_equals_uploaded_mirror():
    run_sequence("yard")


def test_rebuild_sequence_product_default_threaded_wide():
    run_sequence("yard", flags=0, default_traversal=True)


def test_rebuild_sequence_small_scene():
    run_sequence("small", size=(80, 56))


def test_rebuild_sequence_vs_oracle():
    """The oracle fed the mirror scene (mesh level: the builder's rebuilt trees) on the device's instance-level tree shapes, as
    test_deform_sequence_vs_oracle does."""
    from oracle_lib import oracle_plugin
    from test_device_refit import refit_nodes

    gpu, _, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cpu = oracle_plugin()
    cpu.set_scene(twin_scene)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for n in range(1, 5):
        if n > 1:
            data, joints = folded_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            rebuild = NAMES if n in (2, 4) else ()
            for name in rebuild:
                gpu.engine.rebuild_mesh_tree(dev_meshes[name]["index"])
            new = mirror(twin_scene.builder, twin_meshes, data, rebuild)
            topo_t, topo_l = gpu.engine.read_trees(len(new.instance_nodes), len(new.emissive_nodes))
            boxes = np.array([[list(i.min), list(i.max)] for i in new.instances], dtype=np.float32)
            eboxes = np.array([[[e.position[k] - e.radius for k in range(3)], [e.position[k] + e.radius for k in range(3)]] for e in new.emissives], dtype=np.float32)
            cpu.set_scene(hk.SceneData(previous_transforms=new.previous_transforms, vertices=new.vertices, primitives=new.primitives, asset_nodes=new.asset_nodes,
                                       materials=new.materials, instances=new.instances, instance_nodes=refit_nodes(topo_t, boxes), emissives=new.emissives,
                                       emissive_nodes=refit_nodes(topo_l, eboxes), alias_table=new.alias_table))
        for p in (gpu, cpu):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(cpu))
        assert bad == {}, f"frame {n}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- links at size
def soup(k, seed):
    """k small separate triangles in a box, and the same soup folded about x = 0"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (k, 1, 3))
    p = (c + rng.uniform(-0.05, 0.05, (k, 3, 3))).reshape(-1, 3).astype(np.float32)
    return p, S.folded_cloth(p, gap=0.1)[0], np.arange(3 * k, dtype=np.uint32)


def sized_meshes():
    out = {f"{k}": soup(k, k) for k in (1, 2, 3, 1023, 1024, 1025)}
    p, _, _, idx = big_mesh()
    out["130051"] = (p, S.folded_cloth(big_mesh_frame(p, 1), gap=0.01)[0], idx)
    hp, hidx = half_split_mesh(2500)
    out["half_split"] = ((hp * np.float32(1.25) + np.float32(0.5)).astype(np.float32), hp, hidx)
    # ... and beyond SAH_WIDE_MIN: every level of the multi-workgroup top takes the half split (no bucket pass, no carry)
    hp, hidx = half_split_mesh(40000, step=2.0 ** -10)
    out["half_split_40000"] = ((hp * np.float32(1.25) + np.float32(0.5)).astype(np.float32), hp, hidx)
    # a soup beyond SAH_WIDE_MIN in which every triangle comes three times: the copies share a centre, so they are told apart by the
    # half split of their index list alone - the order the stable re-order of the levels above left them in
    p, q, i = soup(14000, 5)
    tri = i.reshape(-1, 3)
    out["triplicated_42000"] = (p, q, np.concatenate([tri, tri, tri]).reshape(-1).astype(np.uint32))
    return out


def scene_with(positions, idx):
    """a bystander cloth, the mesh under test, a bystander sphere: (scene, builder, mesh id)"""
    b = SceneBuilder()
    mat = b.add_material(S.standard_material((0.7, 0.7, 0.7, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    p, n, uv, i = S.cloth_grid(5, 4)
    ids = [b.add_mesh(p, n, uv, i)]
    n, uv = flat(positions)
    mesh = b.add_mesh(positions, n, uv, idx)
    ids.append(mesh)
    p, n, uv, i = S._sphere(5, 6)
    ids.append(b.add_mesh(p, n, uv, i))
    for m in ids:
        b.add_instance(m, mat, IDENTITY)
    scene = b.finish()
    scene.builder = b
    return scene, b, mesh


@pytest.mark.parametrize("threaded", [False, True])
@pytest.mark.parametrize("name", ["1", "2", "3", "1023", "1024", "1025", "130051", "half_split", "half_split_40000", "triplicated_42000"])
def test_device_links_equal_a_fresh_build(name, threaded):
    rest, new, idx = SIZED[name]

    def plugin():
        if threaded:
            with product_default_traversal():
                return hk.HikariPlugin(device=0, flags=0)
        return hk.HikariPlugin(device=0)

    scene, b, mesh = scene_with(rest, idx)
    index = b.mesh_index(mesh)
    gpu, twin, fresh = plugin(), plugin(), plugin()
    gpu.set_scene(scene)
    before = np.frombuffer(bytes(gpu.engine.read_mesh_nodes()[0]), NODE).copy()
    # a rebuild before any deformation: the triangle boxes are produced first, the tree is the one the host built
    gpu.engine.rebuild_mesh_tree(index, F.TREE_SAH)
    a, count, orderings = gpu.engine.read_mesh_nodes()
    assert orderings in ((1, 8) if threaded else (1,))   # (a scene inside the LDS copy keeps one ordering)
    same = np.frombuffer(bytes(a), NODE)
    assert np.array_equal(same["entry"], before["entry"]) and np.array_equal(same["exit"], before["exit"]), "a rebuild without a deformation changed the links"
    assert np.array_equal(same["min"], before["min"]) and np.array_equal(same["max"], before["max"])   # (by value: the union's zeros may carry the other sign)
    gpu.engine.update_mesh_vertices(index, new)
    gpu.engine.rebuild_mesh_tree(index, F.TREE_SAH)
    first = bytes(gpu.engine.read_mesh_nodes()[0])
    gpu.engine.rebuild_mesh_tree(index, F.TREE_SAH)
    assert bytes(gpu.engine.read_mesh_nodes()[0]) == first, "two rebuilds in a row differ"
    # the mirror, uploaded
    b.set_mesh_vertices(mesh, new)
    b.rebuild_mesh_tree(mesh)
    twin.set_scene(b.finish())
    assert bytes(twin.engine.read_mesh_nodes()[0]) == first, "mesh-level nodes differ from the uploaded mirror's"
    # a fresh add_mesh over the same positions: the same links node for node in every ordering, the same boxes by value
    fscene, fb, fmesh = scene_with(new, idx)
    fresh.set_scene(fscene)
    got = np.frombuffer(first, NODE).reshape(orderings, count)
    want = np.frombuffer(bytes(fresh.engine.read_mesh_nodes()[0]), NODE).reshape(orderings, count)
    lo, hi = index.node_offset, index.node_offset + index.node_count
    assert np.array_equal(got["entry"][:, lo:hi], want["entry"][:, lo:hi]) and np.array_equal(got["exit"][:, lo:hi], want["exit"][:, lo:hi])
    assert np.array_equal(got["min"][:, lo:hi], want["min"][:, lo:hi]) and np.array_equal(got["max"][:, lo:hi], want["max"][:, lo:hi])
    # the other meshes: untouched bytes
    was = before.reshape(orderings, count)
    assert got[:, :lo].tobytes() == was[:, :lo].tobytes() and got[:, hi:].tobytes() == was[:, hi:].tobytes()
    # a deformation after the rebuild refits the NEW shape: same links, the mirror's bytes
    again = (new * np.float32(0.75)).astype(np.float32)
    gpu.engine.update_mesh_vertices(index, again)
    b.set_mesh_vertices(mesh, again)
    twin.set_scene(b.finish())
    assert bytes(gpu.engine.read_mesh_nodes()[0]) == bytes(twin.engine.read_mesh_nodes()[0]), "the refit after the rebuild differs from the mirror's"


SIZED = sized_meshes()


# ---------------------------------------------------------------------------------------------------------------- emitters
def test_emitter_records_stay_and_frames_equal_the_twin():
    """A deformed 3 840-triangle emissive sphere rebuilt: the mesh box and the triangle order stay, so do the emitter records and the
    alias table; frames equal the twin's."""
    def glowing():
        scene, sun = S.synthetic_scene(n_boxes=6, n_spheres=2, n_emitters=1, sphere_rings=6, sphere_segs=8)
        b = scene.builder
        p, n, uv, idx = S._sphere(40, 48)
        mid = b.add_mesh(p, n, uv, idx)
        glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
        b.add_instance(mid, glow, S._trs((0.8, 1.8, -0.4), (0.2, 0.1, 0.0), (0.5, 0.4, 0.6)))
        scene = b.finish()
        scene.builder = b
        return scene, sun, mid, p, n

    (dev, sun, mid, rest, nrm), (tw, _, tmid, _, _) = glowing(), glowing()
    index = dev.builder.mesh_index(mid)
    assert index.node_count == 3 * 3840 - 2
    gpu, twin = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER), hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    gpu.set_scene(dev)
    twin.set_scene(tw)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for n in range(1, 4):
        if n > 1:
            q = (S.pulsing_sphere(rest, n) * np.array([1.0, 1.0 + 0.2 * n, 1.0], np.float32)).astype(np.float32)
            gpu.engine.update_mesh_vertices(index, q)
            ra, aa = gpu.engine.read_emitters()
            gpu.engine.rebuild_mesh_tree(index)
            rb, ab = gpu.engine.read_emitters()
            assert ra.tobytes() == rb.tobytes() and aa.tobytes() == ab.tobytes(), "the rebuild moved an emitter record or the alias table"
            tw.builder.set_mesh_vertices(tmid, q)
            tw.builder.rebuild_mesh_tree(tmid)
            twin.set_scene(tw.builder.finish())
            rt, at = twin.engine.read_emitters()
            assert rb.tobytes() == rt.tobytes() and ab.tobytes() == at.tobytes()
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- frames in flight
def test_eight_frames_in_flight_with_a_rebuild_between_each():
    """Eight frames enqueued without a host wait, a deformation and a rebuild between each: the last frame equals the twin's, which
    was given the mirror of the last state (its history: the same frames, rendered one at a time from mirrors)."""
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    for n in range(1, 9):
        if n > 1:
            data, joints = folded_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            for name in NAMES:
                gpu.engine.rebuild_mesh_tree(dev_meshes[name]["index"])
        gpu.render(cam, s, lights=lights, frame_number=n)
    for n in range(1, 9):
        if n > 1:
            data, _ = folded_data(twin_meshes, n)
            twin.set_scene(mirror(twin_scene.builder, twin_meshes, data, NAMES))
        twin.render(cam, s, lights=lights, frame_number=n)
        twin.engine.wait()
    bad = diff_buffers(snapshot(gpu), snapshot(twin))
    assert bad == {}, bad
    nodes_equal(gpu, twin, "after eight frames")


def test_many_rebuilds_between_frames_never_wait_for_the_device():
    """Rebuild calls between two frames only enqueue: with a long frame still running on the device, ten deformations each followed by
    a rebuild return long before it ends (a call that waited for the device - a synchronisation, a scratch grown on every call - would
    take the frame's time).  Built like test_many_deformations_between_frames_never_wait_for_the_device."""
    import time

    scene, sun, meshes = S.deforming_scene("yard")
    p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    p.set_scene(scene)
    cam, lights = synthetic_camera(1920, 1080), hk.lights_uniform(directional=sun)
    s = hk.HikariSettings(indirect_bounces=8, upscale=hk.Upscale.SMAA_TU_1_0)
    p.render(cam, s, lights=lights, frame_number=1)
    p.engine.wait()
    t0 = time.perf_counter()
    p.render(cam, s, lights=lights, frame_number=2)
    p.engine.wait()
    frame_s = time.perf_counter() - t0
    data, _ = folded_data(meshes, 3)
    for warm in range(2):   # (the first round may allocate staging buffers and the build scratch)
        p.render(cam, s, lights=lights, frame_number=3 + warm)
        t0 = time.perf_counter()
        for k in range(10):
            p.engine.update_mesh_vertices(meshes["cloth"]["index"], *data["cloth"])
            p.engine.rebuild_mesh_tree(meshes["cloth"]["index"], F.TREE_SAH if k % 2 == 0 else F.TREE_LBVH)
        calls_s = time.perf_counter() - t0
        p.engine.wait()
    assert calls_s < 0.5 * frame_s, (calls_s, frame_s)


# ---------------------------------------------------------------------------------------------------------------- LBVH
def unfold(nodes):
    """device nodes of one tree (ordering 0) back in the builder's layout: a navigator that took over its single leaf's role points at the
    leaf again, leaves carry the empty box"""
    a = nodes.copy()
    for k in range(len(a) - 1):
        if a["entry"][k] >= LEAF and a["entry"][k + 1] == a["entry"][k] and a["exit"][k + 1] == a["exit"][k]:
            a["entry"][k] = k + 1
    return a


def test_lbvh_rebuild_gives_a_valid_tree_and_frames_equal_a_twin_given_that_tree():
    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    data, joints = folded_data(dev_meshes, 3)
    deform_device(gpu.engine, dev_meshes, data, joints)
    cl = dev_meshes["cloth"]
    gpu.engine.rebuild_mesh_tree(cl["index"], F.TREE_LBVH)
    raw, count, orderings = gpu.engine.read_mesh_nodes()
    dev = np.frombuffer(bytes(raw), NODE).reshape(orderings, count)
    lo, hi = cl["index"].node_offset, cl["index"].node_offset + cl["index"].node_count
    tree = dev[0, lo:hi]
    n_tris = (cl["index"].node_count + 2) // 3
    idx = S.cloth_grid(12, 12, size=2.0)[3].reshape(-1, 3).astype(np.int64)
    tris = data["cloth"][0][idx]
    tlo, thi = tris.min(axis=1), tris.max(axis=1)
    a = unfold(tree)
    leaf = a["entry"] >= LEAF
    assert sorted((a["entry"][leaf] - LEAF).tolist()) == list(range(n_tris)), "every triangle exactly once"
    for i in np.flatnonzero(~leaf):   # every navigator: the union of the leaves of its range
        assert a["entry"][i] == i + 1 and i + 1 < a["exit"][i] <= len(a)
        shapes = (a["entry"][i + 1:a["exit"][i]][leaf[i + 1:a["exit"][i]]] - LEAF).astype(np.int64)
        assert np.array_equal(a["min"][i], tlo[shapes].min(axis=0)) and np.array_equal(a["max"][i], thi[shapes].max(axis=0)), i
    # the twin: the mirror of the deformation, with the read-back ordering-0 tree as the cloth's asset nodes
    new = mirror(twin_scene.builder, twin_meshes, data)
    nodes = node_array(new.asset_nodes)
    a["min"][leaf], a["max"][leaf] = np.float32(np.inf), np.float32(-np.inf)
    nodes[lo:hi] = a
    carried = (F.HkNode * len(nodes)).from_buffer_copy(nodes.tobytes())
    twin.set_scene(hk.SceneData(previous_transforms=new.previous_transforms, vertices=new.vertices, primitives=new.primitives, asset_nodes=carried, materials=new.materials,
                                instances=new.instances, instance_nodes=new.instance_nodes, emissives=new.emissives, emissive_nodes=new.emissive_nodes,
                                alias_table=new.alias_table))
    for n in (1, 2, 3):
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- bands
@pytest.mark.parametrize("bands,bounds", [(2, [0, 20, 64]), (3, [0, 9, 40, 64])])
def test_bands_rebuilding_equal_the_single_context(bands, bounds):
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
            data, joints = folded_data(meshes, n)
            for t in (m, ref):
                deform_device(t, meshes, data, joints)
                if n != 3:
                    for name in NAMES:
                        t.rebuild_mesh_tree(meshes[name]["index"], F.TREE_SAH)
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        m.wait(); ref.wait()
        for b in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(b).view(np.uint8) == ref.read(b).view(np.uint8)).all(), f"{bands} bands, frame {n}: buffer {b} differs"


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing_and_stale_mirrors_are_refused():
    scene, sun, meshes = S.deforming_scene("yard")
    p = hk.HikariPlugin(device=0)
    api = p.engine.api
    cl = meshes["cloth"]
    assert api.raw("rebuild_mesh_tree")(p.engine.ctx, C.byref(cl["index"]), F.TREE_SAH) == F.HK_E_NOT_READY   # no scene yet
    p.set_scene(scene)
    ctx = p.engine.ctx
    before = bytes(p.engine.read_mesh_nodes()[0])
    bad = F.HkMeshIndex(cl["index"].vertex, cl["index"].primitive, cl["index"].node_offset + 1, cl["index"].node_count)
    assert api.raw("rebuild_mesh_tree")(ctx, C.byref(bad), F.TREE_SAH) == F.HK_E_INVALID
    assert api.raw("rebuild_mesh_tree")(ctx, C.byref(cl["index"]), 2) == F.HK_E_INVALID
    assert api.raw("rebuild_mesh_tree")(ctx, None, F.TREE_SAH) == F.HK_E_INVALID
    huge = F.HkMeshIndex(cl["index"].vertex, cl["index"].primitive, cl["index"].node_offset, 3 * 4194305 - 2)
    assert api.raw("rebuild_mesh_tree")(ctx, C.byref(huge), F.TREE_SAH) == F.HK_E_INVALID   # (an unknown record first, whatever its size)
    assert bytes(p.engine.read_mesh_nodes()[0]) == before
    b = scene.builder
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_OK   # nothing was written: no mirror is stale
    # a rebuild makes the host mirrors stale, like a deformation
    cam, lights, s = synthetic_camera(64, 48), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    p.render(cam, s, lights=lights, frame_number=1)
    data, _ = folded_data(meshes, 3)
    p.engine.update_mesh_vertices(cl["index"], *data["cloth"])
    b.set_mesh_vertices(cl["id"], *data["cloth"])
    p.set_scene(b.finish())   # the deformation's mirror is up: only the rebuild stands between host and device from here
    p.engine.rebuild_mesh_tree(cl["index"])
    inst = scene.instances
    assert api.raw("upload_instances")(ctx, inst, len(inst), scene.instance_nodes, len(scene.instance_nodes), scene.emissives, len(scene.emissives), scene.emissive_nodes,
                                       len(scene.emissive_nodes), scene.alias_table, len(scene.alias_table)) == F.HK_E_NOT_READY
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_E_NOT_READY
    p.render(cam, s, lights=lights, frame_number=2)
    mode, orderings = C.c_uint32(), C.c_uint32()
    assert api.raw("upload_materials")(ctx, scene.materials, len(scene.materials)) == F.HK_OK   # taken; the next use of the scene refuses the stale layout
    assert api.raw("traversal_mode")(ctx, C.byref(mode), C.byref(orderings)) == F.HK_E_NOT_READY
    b.rebuild_mesh_tree(cl["id"])
    p.set_scene(b.finish())
    assert api.raw("upload_scene_instances")(ctx, b.h) == F.HK_OK
    p.render(cam, s, lights=lights, frame_number=3)


def test_cloth_in_the_cornell_box_leaves_the_one_level_walk_at_the_rebuild():
    def cornell_cloth():
        scene = hk.load_cornell()
        b = scene.builder
        p, n, uv, idx = S.cloth_grid(3, 3, size=1.0)
        p = p + np.array([0.0, 1.0, 0.0], np.float32)
        mid = b.add_mesh(p, n, uv, idx)
        b.add_instance(mid, 0, np.ctypeslib.as_array(scene.instances[0].model).copy())
        scene = b.finish()
        scene.builder = b
        return scene, mid, b.mesh_index(mid)

    with product_default_traversal():
        gpu, twin = hk.HikariPlugin(device=0), hk.HikariPlugin(device=0)
    (dev, mid, index), (tw, tmid, _) = cornell_cloth(), cornell_cloth()
    gpu.set_scene(dev)
    twin.set_scene(tw)
    twin.engine.api.call("debug_set_option", twin.engine.ctx, F.DEBUG_OPT_FLAT_WALK, 0)
    cam, s = hk.cornell_camera(96, 64), hk.HikariSettings(**SETTINGS)

    def mode(p):
        m, o = C.c_uint32(), C.c_uint32()
        p.engine.api.call("traversal_mode", p.engine.ctx, C.byref(m), C.byref(o))
        return m.value & 0xFF

    assert mode(gpu) == 2   # HK_TRAVERSAL_ONE_LEVEL
    for n in (1, 2, 3):
        if n == 2:
            gpu.engine.rebuild_mesh_tree(index)
            assert mode(gpu) == 0   # HK_TRAVERSAL_REFERENCE
            tw.builder.rebuild_mesh_tree(tmid)
            twin.set_scene(tw.builder.finish())
        for p in (gpu, twin):
            p.render(cam, s, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"
    dev.builder.rebuild_mesh_tree(mid)
    gpu.set_scene(dev.builder.finish())
    assert mode(gpu) == 2
