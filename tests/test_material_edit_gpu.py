"""Material edits on the device (hk_update_materials).  Twin builders, as in test_device_refit.py: the device context is fed its
builder through hk_update_materials, the CPU oracle the twin builder's records - materials first, then the instance level.
  case A (the emitting set stays): the oracle gets the twin's finish() emitters on the OLD light-tree shape, every inner box re-derived
          as the union of the leaves below it (the refit), and the instance tree it had;
  case B (an emitter switched on or off): the oracle gets the twin's full finish(), the reference's path; the trees the device builds
          (HK_TREE_SAH) must be the twin's, link for link.
HK_CTX_DETERMINISTIC_SCATTER, 2 bounces: every buffer of every frame bit for bit."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd.distributed import MultiEngine
from bevy_hikari_amd.plugin import SceneData
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_scene
from cases import assert_rendered_within, diff_buffers, product_default_traversal, snapshot
from test_device_refit import LARGE, SMALL, oracle, pose, refit_nodes, same_links

pytestmark = pytest.mark.gpu
SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
EMITTER_MATERIAL = 8   # synthetic_scene: materials 0..7 plain, 8.. the emitters' own
MOVERS = lambda n: [2, 7, 22, n - 1]


def copy_of(m):
    out = F.HkMaterial()
    C.memmove(C.byref(out), C.byref(m), C.sizeof(F.HkMaterial))
    return out


def plain(frame, k):
    def f(m):
        m.base_color[:] = [0.15 + 0.1 * frame, 0.9 - 0.12 * frame, 0.3 + 0.05 * k, 1.0]
        m.perceptual_roughness, m.metallic = 0.3 + 0.1 * frame, float((frame + k) % 2)
    return f


def glow(frame):
    def f(m):   # colour and alpha of an emitter that stays one: dim at frame 2 (a radius of about 2, well inside the yard), then four
        # times the intensity per frame - the radius, and with it the light tree's boxes, moves through the scene
        m.emissive[:] = [1.0 - 0.1 * frame, 0.3 + 0.1 * frame, 0.5, 0.004 * 4.0 ** (frame - 1)]
    return f


def fade(frame):
    def f(m):   # a gentler change (the light tree a host would BUILD for it keeps its shape: test_after_a_deformation compares with one)
        m.emissive[:] = [1.0 - 0.15 * frame, 0.3 + 0.1 * frame, 0.5, 1.0 - 0.12 * frame]
    return f


def off(m):
    m.emissive[:] = [0.0, 0.0, 0.0, 1.0]


def on(m):
    m.emissive[:] = [0.9, 0.5, 0.3, 0.8]


def case_a(frame, plain_ids=(1, 2), emitter=EMITTER_MATERIAL):
    return {plain_ids[0]: plain(frame, 0), plain_ids[1]: plain(frame, 1), emitter: glow(frame)}


def apply_edits(builders, materials, edits):
    """edits {material id: callable(HkMaterial)} on the running list `materials`, set on every builder; returns the count."""
    for i, f in edits.items():
        m = copy_of(materials[i])
        f(m)
        materials[i] = m
        for b in builders:
            b.set_material(i, m)
    return len(edits)


def material_array(materials):
    arr = (F.HkMaterial * len(materials))()
    for i, m in enumerate(materials):
        C.memmove(C.byref(arr[i]), C.byref(m), C.sizeof(F.HkMaterial))
    return arr


def boxes_of(scene):
    boxes = np.array([[list(i.min), list(i.max)] for i in scene.instances], dtype=np.float32)
    eboxes = np.array([[[e.position[k] - e.radius for k in range(3)], [e.position[k] + e.radius for k in range(3)]] for e in scene.emissives], dtype=np.float32)
    return boxes, eboxes


def emitting(scene):
    return [e.instance for e in scene.emissives]


class Twin:
    """The twin builder and what the device must hold after each update: feeds the oracle (or any context) through `feed`."""

    def __init__(self, scene):
        self.scene, self.builder = scene, scene.builder
        self.materials = [copy_of(m) for m in scene.materials]
        self.topo_tlas, self.topo_light = scene.instance_nodes, scene.emissive_nodes
        self.rest = np.array([np.ctypeslib.as_array(i.model).copy() for i in scene.instances], dtype=np.float32)
        self.current = self.rest.copy()
        self.last = scene

    def move(self, builders, movers, frame):
        self.previous = self.current.copy()
        for k, i in enumerate(movers):
            self.current[i] = pose(self.rest[i], frame - 1, k)
            for b in builders:
                b.set_instance_transform(i, self.current[i])

    def expected(self):
        """-> (case, SceneData): what the device holds after hk_update_materials (+ the refit of this frame's movers)"""
        new = self.builder.finish()
        case = "B" if emitting(new) != emitting(self.last) else "A"
        self.last = new
        if case == "B":
            self.topo_tlas, self.topo_light = new.instance_nodes, new.emissive_nodes
            return case, new
        boxes, eboxes = boxes_of(new)
        return case, SceneData(previous_transforms=getattr(self, "previous", self.current).copy(), vertices=new.vertices, primitives=new.primitives, asset_nodes=new.asset_nodes,
                               materials=new.materials, instances=new.instances, instance_nodes=refit_nodes(self.topo_tlas, boxes), emissives=new.emissives,
                               emissive_nodes=refit_nodes(self.topo_light, eboxes) if len(new.emissives) else new.emissive_nodes, alias_table=new.alias_table)


def feed(plugin, scene):
    """materials, then the instance level: the order the reference prepares them in"""
    plugin.engine.api.call("upload_materials", plugin.engine.ctx, scene.materials, len(scene.materials))
    plugin.update_instances(scene)


def run_sequence(kw, size, plan, frames=5, movers=None, default_traversal=False, within=False, also=None):
    """plan: {frame: {material id: edit}}; also: {frame: callable(builder)}, another edit of both builders in that frame.
    Returns (gpu plugin, Twin, cases per frame)."""
    make = kw if callable(kw) else (lambda: synthetic_scene(**kw))
    dev_scene, sun = make()
    ref_scene, _ = make()
    s = hk.HikariSettings(**SETTINGS)
    cam, lights = synthetic_camera(*size), hk.lights_uniform(directional=sun)
    if default_traversal:
        with product_default_traversal():
            gpu = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    else:
        gpu = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    cpu = oracle()
    gpu.set_scene(dev_scene)
    cpu.set_scene(ref_scene)
    twin = Twin(ref_scene)
    builders = (dev_scene.builder, ref_scene.builder)
    cases, uploads = {}, None
    for n in range(1, frames + 1):
        if n > 1 and (n in plan or movers):
            if movers:
                twin.move(builders, movers, n)
            for b in builders if also and n in also else ():
                also[n](b)
            edited = apply_edits(builders, twin.materials, plan.get(n, {}))
            radius_before = {e.instance: e.radius for e in twin.last.emissives}
            changed = gpu.engine.update_materials(dev_scene.builder, F.TREE_SAH)   # first: case B takes the motion along
            assert changed == edited, f"frame {n}: {changed} records changed, {edited} edited"
            case, want = twin.expected()
            cases[n] = case
            moved = gpu.engine.refit_instances(dev_scene.builder) if movers else 0
            assert moved == (0 if case == "B" or not movers else len(movers)), f"frame {n}: case {case}, {moved} moved"
            if case == "B":
                tlas, light = gpu.engine.read_trees(len(want.instance_nodes), len(want.emissive_nodes))
                assert same_links(tlas, want.instance_nodes), f"frame {n}: instance tree differs from the host's bvh 0.7.1 build"
                assert same_links(light, want.emissive_nodes), f"frame {n}: light tree differs from the host's bvh 0.7.1 build"
            elif EMITTER_MATERIAL in plan.get(n, {}) and len(want.emissives):   # the premise: the edit reaches the emitter's radius
                assert any(np.float32(e.radius).tobytes() != np.float32(radius_before[e.instance]).tobytes() for e in want.emissives), f"frame {n}: no radius changed"
            feed(cpu, want)
        for p in (gpu, cpu):
            p.render(cam, s, lights=lights, frame_number=n)
        if within:
            assert_rendered_within(snapshot(gpu), snapshot(cpu), f"frame {n}")
        else:
            bad = diff_buffers(snapshot(gpu), snapshot(cpu))
            assert bad == {}, f"frame {n} ({cases.get(n, '-')}): {bad}"
        if n == 1:
            uploads = gpu.engine.stats().scene_instance_builds
    gpu.uploads_after_frame_1 = uploads
    return gpu, twin, cases


def assert_emitters_equal(gpu, scene):
    rec, _ = gpu.engine.read_emitters()
    want = np.array([[e.position[0], e.position[1], e.position[2], e.radius] for e in scene.emissives], dtype=np.float32)
    assert rec[:, :4].tobytes() == want.tobytes(), "position / radius of the device's emitters differ from the twin builder's"


@pytest.mark.parametrize("which", ["small", "large"])
def test_case_a_against_the_oracle(which):
    """From frame 2 on every frame changes two non-emissive materials and the colour and alpha of one emitter's material."""
    kw, size = (SMALL, (88, 60)) if which == "small" else (LARGE, (120, 72))
    gpu, twin, cases = run_sequence(kw, size, {n: case_a(n) for n in range(2, 6)})
    assert set(cases.values()) == {"A"}
    st = gpu.engine.stats()
    assert st.scene_instance_builds == gpu.uploads_after_frame_1, "the instance-level arrays must not have been laid out again on the host"
    assert st.scene_device_tree_builds == 0 and st.scene_device_refits == 0
    assert_emitters_equal(gpu, twin.last)


def test_edits_while_objects_move():
    """The same edits plus hk_refit_scene_instances of four movers in the same frames, hk_update_materials first.  In the state this
    leaves (the host copies are stale) hk_upload_materials is still refused at the next frame - hk_update_materials is not."""
    n = 1 + 20 + 5 + 3
    gpu, twin, cases = run_sequence(LARGE, (120, 72), {f: case_a(f) for f in range(2, 6)}, movers=MOVERS(n))
    assert set(cases.values()) == {"A"}
    st = gpu.engine.stats()
    assert st.scene_device_refits == 4 and st.scene_instance_builds == gpu.uploads_after_frame_1
    assert_emitters_equal(gpu, twin.last)
    e, b = gpu.engine, twin.builder   # (the twin builder holds the same values as the device's: it serves as the host's here)
    apply_edits((b,), twin.materials, case_a(6))
    assert e.update_materials(b) == 3                                    # HK_OK in the state refused below
    e.api.call("upload_materials", e.ctx, material_array(twin.materials), len(twin.materials))
    with pytest.raises(hk.HikariError) as err:
        gpu.render(synthetic_camera(120, 72), hk.HikariSettings(**SETTINGS), frame_number=6)
    assert err.value.code == F.HK_E_NOT_READY


def test_a_material_shared_by_several_instances():
    """The strip quad and two emissive spheres share ONE emissive material: every emitter of it is re-derived."""
    kw = dict(n_emissive_spheres=2, **SMALL)
    scene, _ = synthetic_scene(**kw)
    sharing = [e.instance for e in scene.emissives if scene.instances[e.instance].material == EMITTER_MATERIAL]
    assert len(sharing) == 3, "the premise: three emitters of one material"
    before = {e.instance: e.radius for e in scene.emissives}
    gpu, twin, cases = run_sequence(kw, (88, 60), {n: case_a(n) for n in range(2, 5)}, frames=4)
    assert set(cases.values()) == {"A"}
    assert all(e.radius != before[e.instance] for e in twin.last.emissives)
    assert_emitters_equal(gpu, twin.last)


def test_case_b_small_scene_the_only_emitter_off_and_on_again():
    gpu, twin, cases = run_sequence(SMALL, (88, 60), {2: {EMITTER_MATERIAL: off}, 4: {EMITTER_MATERIAL: on}})
    assert cases == {2: "B", 4: "B"}
    assert len(twin.last.emissives) == 1
    assert gpu.engine.stats().scene_device_tree_builds == 2   # (the case-B calls only; frame 2 leaves six instances and NO emitter)


def test_case_b_large_scene_with_movers():
    """One of three emitters off at frame 2, a box material made emissive at frame 3, four movers in both frames - and a case-A edit on
    the new emitter list at frame 4."""
    n = 1 + 20 + 5 + 3
    scene, _ = synthetic_scene(**LARGE)
    box_material = scene.instances[3].material
    plan = {2: {EMITTER_MATERIAL + 1: off}, 3: {box_material: on}, 4: case_a(4, plain_ids=(0, box_material))}
    gpu, twin, cases = run_sequence(LARGE, (120, 72), plan, frames=4, movers=MOVERS(n))
    assert cases == {2: "B", 3: "B", 4: "A"}
    st = gpu.engine.stats()
    assert st.scene_device_tree_builds == 2 and st.scene_device_refits == 1
    assert_emitters_equal(gpu, twin.last)


def test_an_instance_reassigned_in_the_builder_travels_with_the_edit():
    """hk_scene_builder_set_instance_material pending in the builder (what hk_refit_scene_instances refuses) next to a value edit that
    leaves the emitting set alone: the call must not take case A, which works from the context's instance records and would drop the
    reassignment - it takes the instance-set path, and the frames equal the oracle's with the instance's new material."""
    scene, _ = synthetic_scene(**SMALL)
    other = next(m for m in range(1, 8) if m != scene.instances[2].material)
    gpu, twin, cases = run_sequence(SMALL, (88, 60), {2: {1: plain(2, 0)}, 3: {1: plain(3, 0)}}, frames=3, also={2: lambda b: b.set_instance_material(2, other)})
    assert twin.last.instances[2].material == other and cases == {2: "A", 3: "A"}   # (the emitting set never changed)
    st = gpu.engine.stats()
    assert st.scene_device_tree_builds == 1, "frame 2 must have gone through hk_update_scene_instances, frame 3 not"


def test_after_a_deformation():
    """Case A after hk_update_mesh_vertices / hk_skin_mesh (the state in which every relayout is refused): frames equal a twin context
    that received hk_upload_scene of the mirrored builder with the new materials.  Case B is refused and changes nothing."""
    from test_mesh_deform_gpu import deform_device, frame_data, make_pair, mirror

    gpu, twin, dev_scene, twin_scene, dev_meshes, twin_meshes, sun = make_pair("yard", F.CTX_DETERMINISTIC_SCATTER)
    cam, lights, s = synthetic_camera(96, 64), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    cloth_material, glow_material = 10, 11   # deforming_scene: after the yard's 8 + 2
    materials = [copy_of(m) for m in dev_scene.materials]
    builders = (dev_scene.builder, twin_scene.builder)
    shape = [(n.entry_index, n.exit_index) for n in twin_scene.emissive_nodes]

    def compare(n):
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"frame {n}: {bad}"

    for n in range(1, 5):
        if n > 1:
            data, joints = frame_data(dev_meshes, n)
            deform_device(gpu.engine, dev_meshes, data, joints)
            edits = {cloth_material: plain(n, 0), glow_material: fade(n), EMITTER_MATERIAL: fade(n + 1)}   # the pulsing sphere's and a quad's
            apply_edits(builders, materials, edits)
            assert gpu.engine.update_materials(dev_scene.builder) == 3
            new = mirror(twin_scene.builder, twin_meshes, data)
            assert [(q.entry_index, q.exit_index) for q in new.emissive_nodes] == shape, "the premise: the twin's light tree keeps its shape"
            twin.set_scene(new)
        compare(n)
    before = copy_of(materials[glow_material])
    apply_edits((dev_scene.builder,), materials, {glow_material: off})
    with pytest.raises(hk.HikariError) as err:
        gpu.engine.update_materials(dev_scene.builder)
    assert err.value.code == F.HK_E_NOT_READY
    dev_scene.builder.set_material(glow_material, before)
    assert gpu.engine.update_materials(dev_scene.builder) == 0    # ... and the context still holds the old values
    compare(5)


def test_refusals_write_nothing():
    scene, sun = synthetic_scene(**SMALL)
    twin_scene, _ = synthetic_scene(**SMALL)
    gpu, twin = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER), hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    gpu.set_scene(scene)
    twin.set_scene(twin_scene)
    cam, lights, s = synthetic_camera(88, 60), hk.lights_uniform(directional=sun), hk.HikariSettings(**SETTINGS)
    e, api, b = gpu.engine, gpu.engine.api, scene.builder
    frame = [0]

    def refused(code, *args):
        changed = C.c_uint32(77)
        with pytest.raises(hk.HikariError) as err:
            api.call("update_materials", *args, C.byref(changed))
        assert err.value.code == code, (err.value.code, code)
        frame[0] += 1
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=frame[0])
        bad = diff_buffers(snapshot(gpu), snapshot(twin))
        assert bad == {}, f"after refusal {frame[0]}: {bad}"

    no_scene = hk.Engine(device=0)
    refused(F.HK_E_NOT_READY, no_scene.ctx, b.h, F.TREE_SAH)                      # no scene
    edited = copy_of(scene.materials[1])   # (an edit pending in the builder throughout)
    plain(3, 0)(edited)
    b.set_material(1, edited)
    refused(F.HK_E_INVALID, None, b.h, F.TREE_SAH)                                # NULL context
    refused(F.HK_E_INVALID, e.ctx, None, F.TREE_SAH)                              # NULL builder
    refused(F.HK_E_INVALID, e.ctx, b.h, 7)                                        # unknown tree mode
    more, _ = synthetic_scene(**SMALL)
    more.builder.add_material(copy_of(scene.materials[1]))
    refused(F.HK_E_INVALID, e.ctx, more.builder.h, F.TREE_SAH)                    # another material count
    textured = copy_of(edited)
    textured.base_color_texture = 0                                               # ... of a scene without textures
    b.set_material(2, textured)
    refused(F.HK_E_INVALID, e.ctx, b.h, F.TREE_SAH)
    b.set_material(2, copy_of(scene.materials[2]))
    from bevy_hikari_amd.scenes import _box

    dirty, _ = synthetic_scene(**SMALL)
    dirty.builder.set_material(1, edited)
    dirty.builder.add_mesh(*_box())                                                # unfinished mesh changes
    refused(F.HK_E_NOT_READY, e.ctx, dirty.builder.h, F.TREE_SAH)
    pending, _ = synthetic_scene(**SMALL)
    pending.builder.add_mesh(*_box(), build_tree=False)
    pending.builder.finish()
    pending.builder.set_material(1, edited)                                        # a deferred mesh whose tree is a stand-in
    refused(F.HK_E_NOT_READY, e.ctx, pending.builder.h, F.TREE_SAH)
    # the edit that was pending all along goes through, on the device and - the host's path - on the twin
    assert e.update_materials(b) == 1
    twin_scene.builder.set_material(1, edited)
    twin.set_scene(twin_scene.builder.finish())
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=frame[0] + 1)
    assert diff_buffers(snapshot(gpu), snapshot(twin)) == {}


def test_product_default_traversal_stays_within_tolerance():
    """LARGE at 160x96 with the product's traversal (threaded orderings, wide records, wavefront schedule): case A, case B (an emitter
    off), case A on the new list, case B (on again) - each frame within the project's 1e-3 rule of the oracle's."""
    plan = {2: case_a(2), 3: {EMITTER_MATERIAL + 1: off}, 4: case_a(4), 5: {EMITTER_MATERIAL + 1: on}}
    gpu, twin, cases = run_sequence(LARGE, (160, 96), plan, default_traversal=True, within=True)
    assert cases == {2: "A", 3: "B", 4: "A", 5: "B"}
    assert gpu.engine.wide_walk() and gpu.engine.stats().wide_stack_lost == 0


@pytest.mark.parametrize("which", ["small", "large"])
def test_bands_equal_the_single_context(which):
    """hk_multi_update_materials with three bands on device 0: the union of the bands equals the single context, plane for plane."""
    from test_multi_gpu import _same_buffers

    kw, (w, h) = (SMALL, (88, 60)) if which == "small" else (LARGE, (120, 72))
    multi_scene, sun = synthetic_scene(**kw)
    single_scene, _ = synthetic_scene(**kw)
    s = hk.HikariSettings(**SETTINGS)
    cam, lights = synthetic_camera(w, h), hk.lights_uniform(directional=sun)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    m, ref = MultiEngine([0] * 3), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    for t, scene in ((m, multi_scene), (ref, single_scene)):
        t.upload_noise(); t.upload_scene(scene); t.resize(w, h, 1.0)
    materials = [copy_of(x) for x in single_scene.materials]
    rest = {1: plain(4, 0), 2: plain(4, 1)}
    if which == "large":
        rest[EMITTER_MATERIAL + 1] = glow(4)   # (the small scene has no emitter left at frame 4)
    plan = {2: case_a(2), 3: {EMITTER_MATERIAL: off}, 4: rest, 5: {EMITTER_MATERIAL: on}}
    for n in range(1, 6):
        if n > 1:
            edited = apply_edits((multi_scene.builder, single_scene.builder), materials, plan[n])
            assert m.update_materials(multi_scene.builder) == edited and ref.update_materials(single_scene.builder) == edited
            n_tlas, n_light = len(single_scene.instance_nodes), 3 * len(ref.read_emitters()[0]) - 2
            want = ref.read_trees(n_tlas, max(n_light, 0))
            for e in m.contexts:
                got = e.read_trees(n_tlas, max(n_light, 0))
                assert all(bytes(a) == bytes(b) for a, b in zip(got, want)), f"frame {n}: a band's trees differ from the single context's"
                assert e.read_emitters()[0].tobytes() == ref.read_emitters()[0].tobytes()
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        _same_buffers(m, ref, n, s, f"materials x3 ({which}) ")
    m.wait()
