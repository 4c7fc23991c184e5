"""hk_change_scene_instances: the instance set changed after mesh deformations and device poses, where hk_update_scene_instances is refused.

Every case keeps a LIVE context - loaded with the two-slot base scene of tests/scene_edit_model.py (the pool meshes of
tests/test_remove_meshes_gpu.py), edited, given the new call - and compares it with a TWIN loaded fresh through hk_upload_scene from a
builder made the way the call's contract says: the same meshes with their CURRENT vertices (read from the live context, given to the twin's
builder through hk_scene_builder_set_mesh_vertices) and tree shapes (hk_scene_builder_rebuild_mesh_tree where the live mesh was rebuilt),
the poses the live device holds (read_instance_transforms), the same instance set and materials, host-built SAH trees.  Compared byte for
byte: the emitter records and alias tables, both trees, the poses, and every screen-space buffer of two 64 x 64 frames rendered from an
empty temporal history on both sides.  An implementation that merely lifted the refusal of the host path would lay out stale boxes, areas
and poses: a variant of the library that took the builder's mesh boxes and poses in place of the device's failed the cases after a
deformation, after device poses, after rebuilds, of the emitter counts, of the instance count, of the mesh nothing references, of the
move and of the launch count.  The side-state case (later edits land on the new ids) re-derives those values through the later edits
themselves: what it holds is that they reach the right instances."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
import scene_edit_model as M
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import SceneBuilder
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from test_add_meshes_gpu import MODES, SUN, plugin
from test_mesh_deform_gpu import SETTINGS

pytestmark = pytest.mark.gpu

BASE = "two_slot"
W = H = 64
GREY, TEXTURED, GLOW, GREEN = 0, 1, 2, 3   # the base scene's materials (scene_edit_model.base_description)


def view():
    return synthetic_camera(W, H), hk.lights_uniform(directional=SUN), hk.HikariSettings(**SETTINGS)


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Side:
    """A context with the base scene, its builder, and what a twin needs to know of the edits: the mesh names in builder order, (mesh name,
    material) per instance, the materials, which meshes were deformed or rebuilt on the device."""

    def __init__(self, threaded, base=BASE):
        d = M.base_description(base)
        self.base, self.threaded = base, threaded
        self.p = plugin(threaded)
        self.e = self.p.engine
        self.b = M.base_builder(base)
        self.names = [n for n, _ in d["meshes"]]
        self.inst = [(n, m) for n, m, _ in d["instances"]]
        self.materials = [M.material(base, k, 0) for k in range(len(d["materials"]))]
        self.textures = [t["rgba"] for t in M.base_textures()]
        self.deformed, self.rebuilt = set(), set()
        self.frame = 0
        self.p.set_scene(M.scene_of(self.b, self.textures))
        self.b.take_origins()   # (the context took the base scene)

    # ---- edits of the builder, mirrored
    def index(self, name):
        return self.b.mesh_index(self.names.index(name))

    def add(self, name, material, pose_seed):
        self.b.add_instance(self.names.index(name), material, M.pose(self.base, pose_seed))
        self.inst.append((name, material))

    def remove(self, k):
        self.b.remove_instance(k)
        del self.inst[k]

    def rematerial(self, k, material):
        self.b.set_instance_material(k, material)
        self.inst[k] = (self.inst[k][0], material)

    def change(self):
        self.e.change_instances(self.b, F.TREE_SAH)
        return self.e.last_instance_change()

    def add_mesh(self, name):
        M.add_pool_mesh(self.b, self.base, name, "host")
        self.b.finish()
        self.e.add_meshes(self.b, F.TREE_SAH)
        self.names.append(name)

    def remove_mesh(self, name):
        assert all(n != name for n, _ in self.inst)
        extent = self.b.remove_mesh(self.names.index(name))
        self.e.remove_meshes([extent])
        self.b.finish()
        self.names.remove(name)
        self.deformed.discard(name)
        self.rebuilt.discard(name)

    # ---- what makes the mirrors stale
    def deform(self, kind, name, seed):
        e, idx, d = self.e, self.index(name), M.pool(self.base, name)
        if kind == "vertices":
            e.update_mesh_vertices(idx, *M.vertex_data(self.base, name, seed, True))
        elif kind == "skin":
            e.set_mesh_skin(idx, d["positions"], d["normals"], d["joints"], d["weights"])
            e.deform_meshes([("skin", idx, M.joints(seed))])
        elif kind == "morph_skin":
            e.set_mesh_skin(idx, d["positions"], d["normals"], d["joints"], d["weights"])
            e.set_mesh_morph_targets(idx, *M.morph_set(self.base, name))
            e.deform_meshes([("morph_skin", idx, M.joints(seed), M.morph_weights(seed + 1))])
        else:
            raise KeyError(kind)
        self.deformed.add(name)

    def device_poses(self, seeds, ids=None):
        """poses from a device tensor: `seeds` one pose seed per named instance (ids None: every instance)"""
        poses = np.stack([M.pose(self.base, s) for s in seeds])
        self.e.set_instance_transforms(self.b, cuda(poses), ids)

    def render(self):
        cam, lights, s = view()
        self.frame += 1
        self.p.render(cam, s, lights=lights, frame_number=self.frame)

    def settle(self):
        """in front of a comparison that follows pose calls, refits of the trees or emitter edits: every instance at rest (its current pose
        given twice from a device tensor) and both trees rebuilt over the current boxes, as the closing step of
        tests/test_scene_edit_sequences_gpu.py"""
        poses = cuda(self.e.read_instance_transforms(len(self.inst)))
        for _ in range(2):
            self.e.set_instance_transforms(self.b, poses)
        self.e.rebuild_trees(F.TREE_SAH)


def twin_of(side):
    """(plugin, finished builder) of a fresh context loaded with what the contract says the live one holds"""
    tb = SceneBuilder()
    for m in side.materials:
        tb.add_material(m)
    poses = side.e.read_instance_transforms(len(side.inst))
    instanced = {n for n, _ in side.inst}
    for name in side.names:
        mid = M.add_pool_mesh(tb, side.base, name, "host")
        if name in side.deformed and name in instanced:   # (a mesh nothing references is named by no record: nothing reads its vertices)
            g = side.e.read_mesh_geometry(side.index(name))
            tb.set_mesh_vertices(mid, g["positions"], g["normals"])
        if name in side.rebuilt:
            tb.rebuild_mesh_tree(mid)
    for k, (name, material) in enumerate(side.inst):
        tb.add_instance(side.names.index(name), material, poses[k])
    p = plugin(side.threaded)
    p.set_scene(M.scene_of(tb, side.textures))
    return p, tb


def same_scene_state(a, b, tb, what):
    """emitters, both trees and poses of two engines, byte for byte"""
    scene = tb.scene()
    counts = (len(scene.instance_nodes), len(scene.emissive_nodes))
    for part, g, w in zip(("records", "alias table"), a.read_emitters(), b.read_emitters()):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: the emitters' {part} differ"
    for tree, g, w in zip(("instance tree", "light tree"), a.read_trees(*counts), b.read_trees(*counts)):
        assert bytes(g) == bytes(w), f"{what}: the {tree} differs"
    n = len(scene.instances)
    assert a.read_instance_transforms(n).tobytes() == b.read_instance_transforms(n).tobytes(), f"{what}: the poses differ"
    return scene


def same_frames(pa, pb, what):
    """two frames from an empty temporal history on both sides, every screen-space buffer"""
    cam, lights, s = view()
    for p in (pa, pb):
        p.reset_history()
    for n in (1, 2):
        for p in (pa, pb):
            p.render(cam, s, lights=lights, frame_number=n)
        bad = diff_buffers(snapshot(pa), snapshot(pb))
        assert bad == {}, f"{what}, frame {n}: {bad}"


def against_twin(side, what, emitters=None):
    twin, tb = twin_of(side)
    scene = same_scene_state(side.e, twin.engine, tb, what)
    assert len(scene.instances) == len(side.inst)
    if emitters is not None:
        assert len(scene.emissives) == emitters, f"{what}: the twin has {len(scene.emissives)} emitters"
    same_frames(side.p, twin, what)
    return scene


def the_edits(side, deformed_mesh):
    """an instance of the deformed mesh, one of a rigid mesh, one of the 1 100-triangle soup; the last, a middle and the first instance
    leave; one survivor takes another material.  Leaves [cloth, cylinder, sphere, deformed mesh, s7] from the base's five."""
    side.add(deformed_mesh, GREY, 101)
    side.add("s7", GREEN, 102)
    side.add("s1100", GREY, 103)
    side.remove(len(side.inst) - 1)
    side.remove(1)
    side.remove(0)
    side.rematerial(0, GREEN)
    report = side.change()
    assert report[1:] == (3, 2, report[3]) and not report[3] & 2, report
    assert [n for n, _ in side.inst] == ["cloth", "cylinder", "sphere", deformed_mesh, "s7"]
    return report


# ---------------------------------------------------------------------------------------------------------------- 1: accepted state
@MODES
def test_where_update_instances_is_accepted_the_call_leaves_what_it_leaves(threaded):
    a, b = Side(threaded), Side(threaded)
    for side in (a, b):
        side.render()
        side.add("s7", GREEN, 11)
        side.add("cloth", TEXTURED, 12)
        side.remove(1)
        side.rematerial(0, GREEN)
        side.b.set_instance_transform(2, M.pose(BASE, 13))   # (poses changed on the builder travel with both calls)
    report = a.change()
    assert report[3] & 2 and report[1:3] == (4, 2), report
    b.e.update_instances_on_device(b.b, F.TREE_SAH)
    same_scene_state(a.e, b.e, a.b, "accepted state")
    cam, lights, s = view()
    for n in (2, 3):
        for side in (a, b):
            side.render()
        bad = diff_buffers(snapshot(a.p), snapshot(b.p))
        assert bad == {}, f"accepted state, frame {n}: {bad}"


# ---------------------------------------------------------------------------------------------------------------- 2: after a deformation
@pytest.mark.parametrize("kind,mesh,threaded", [("vertices", "cloth", False), ("vertices", "cloth", True), ("skin", "cylinder", True), ("morph_skin", "cylinder", False)],
                         ids=["vertices-exact", "vertices-default", "skin-default", "morph_skin-exact"])
def test_after_a_deformation(kind, mesh, threaded):
    side = Side(threaded)
    side.render()
    side.deform(kind, mesh, 5)
    side.render()
    assert side.e.api.raw("update_scene_instances")(side.e.ctx, side.b.h, F.TREE_SAH) == F.HK_E_NOT_READY
    the_edits(side, mesh)
    against_twin(side, f"after {kind}", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 3: after device poses
@MODES
def test_after_poses_from_a_device_tensor_survivors_keep_them(threaded):
    side = Side(threaded)
    side.render()
    side.device_poses([201, 202, 203, 204, 205])
    side.render()
    side.device_poses([211, 212], ids=[4, 2])   # (the emitter and the cloth move again: their `moved` flags are set when the call comes)
    before = side.e.read_instance_transforms(5)
    assert side.e.api.raw("update_scene_instances")(side.e.ctx, side.b.h, F.TREE_SAH) == F.HK_E_NOT_READY
    the_edits(side, "cloth")
    after = side.e.read_instance_transforms(5)
    assert after[:3].tobytes() == before[2:5].tobytes(), "the survivors' poses are not the ones the device held"
    assert after[3].tobytes() == M.pose(BASE, 101).tobytes() and after[4].tobytes() == M.pose(BASE, 102).tobytes(), "the new instances' poses are not the builder's"
    against_twin(side, "after device poses", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 4: after rebuilds
def test_after_a_mesh_tree_rebuild_and_a_scene_tree_rebuild():
    side = Side(True)
    side.deform("vertices", "cloth", 9)
    side.e.rebuild_mesh_tree(side.index("cloth"), F.TREE_SAH)
    side.rebuilt.add("cloth")
    side.e.rebuild_trees(F.TREE_SAH)
    side.render()
    the_edits(side, "cloth")
    against_twin(side, "after rebuilds", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 5: emitters
@MODES
def test_the_emitter_count_goes_to_zero_to_one_and_to_two(threaded):
    side = Side(threaded)
    side.add_mesh("s1")
    side.add("s1", GREY, 31)
    assert side.change()[3] & 2   # (still the accepted state)
    side.deform("vertices", "s1", 3)    # a deformed mesh of one triangle
    side.deform("vertices", "s7", 4)    # ... and one of seven
    side.render()
    side.remove(4)                      # the sphere, the scene's one emitter: no light tree
    side.change()
    against_twin(side, "1 -> 0 emitters", emitters=0)
    side.rematerial(4, GLOW)            # the triangle glows: a single leaf, an alias slice of one entry
    side.change()
    scene = against_twin(side, "0 -> 1 emitters", emitters=1)
    assert scene.emissives[0].alias_table[1] == 1
    side.add("s7", GLOW, 32)            # a second emitter: the light tree is built
    side.remove(0)
    side.change()
    scene = against_twin(side, "1 -> 2 emitters", emitters=2)
    assert sorted(e.alias_table[1] for e in scene.emissives) == [1, 7]
    side.rematerial(len(side.inst) - 1, GREY)
    side.change()
    against_twin(side, "2 -> 1 emitters", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 6: instance count
def test_the_instance_count_goes_to_one_and_back():
    side = Side(True)
    for k in (3, 1, 0):
        side.remove(k)
    assert side.change()[3] & 2 and [n for n, _ in side.inst] == ["cloth", "sphere"]
    side.deform("vertices", "cloth", 6)
    side.render()
    side.remove(1)
    assert side.change()[1:3] == (1, 0)
    against_twin(side, "2 -> 1 instances", emitters=0)   # a single leaf: no tree to build
    side.add("sphere", GLOW, 41)
    assert side.change()[1:3] == (1, 1)
    against_twin(side, "1 -> 2 instances", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 7: no instance left
def test_a_deformed_mesh_keeps_its_deformation_while_nothing_references_it():
    side = Side(True)
    side.deform("vertices", "cloth", 8)
    side.render()
    deformed = side.e.read_mesh_geometry(side.index("cloth"))["positions"].copy()
    assert deformed.tobytes() != M.pool(BASE, "cloth")["positions"].tobytes()
    side.remove(2)
    side.change()
    against_twin(side, "the deformed mesh without an instance", emitters=1)
    side.add("cloth", TEXTURED, 51)
    side.change()
    assert side.e.read_mesh_geometry(side.index("cloth"))["positions"].tobytes() == deformed.tobytes()
    against_twin(side, "the deformed mesh with an instance again", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 8: growth
@MODES
def test_a_change_beyond_the_slot_moves_the_scene_behind_the_frames_in_flight(threaded):
    """a host layout's slots hold the layout and 64 B per instance (rounded up to 32 B); an instance takes at least its 208-B record and the
    96 B of its three tree nodes: that many more instances than the room cannot fit"""
    live, still = Side(threaded), Side(threaded)
    for side in (live, still):
        side.deform("vertices", "cloth", 12)
        side.render()
        side.render()
    extra = (64 * len(live.inst) + 31) // (208 + 96) + 1
    still.e.wait()
    for k in range(extra):
        live.add("s7" if k % 2 else "cloth", GREY, 300 + k)
    report = live.change()   # (right behind the frame enqueued above: nothing waited for it)
    assert report[3] == 1 and report[1:3] == (5, extra), report
    bad = diff_buffers(snapshot(live.p), snapshot(still.p))
    assert bad == {}, f"the frame in flight at the move: {bad}"
    against_twin(live, "after the move", emitters=1)
    live.add("cylinder", GREEN, 399)
    report = live.change()
    assert report[3] == 0 and report[1:3] == (5 + extra, 1), ("slots half again the need hold one instance more", report)
    against_twin(live, "after the move, one more", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 9: side state
@MODES
def test_later_edits_land_on_the_new_ids(threaded):
    side = Side(threaded)
    side.deform("skin", "cylinder", 2)
    side.render()
    side.remove(0)                        # every id shifts down by one
    side.add("cylinder", GREEN, 61)
    side.change()
    side.render()
    side.e.deform_meshes([("skin", side.index("cylinder"), M.joints(7))])      # the cylinder's instances are 2 and 4 now
    side.device_poses([71, 72], ids=[3, 1])                                      # the emitter (the sphere) and the cloth
    side.materials[GLOW] = M.material(BASE, GLOW, 1)                             # a case A edit: another emissive colour
    side.b.set_material(GLOW, side.materials[GLOW])
    assert side.e.update_materials(side.b, F.TREE_SAH) == 1
    side.render()
    poses = side.e.read_instance_transforms(5)
    assert poses[3].tobytes() == M.pose(BASE, 71).tobytes() and poses[1].tobytes() == M.pose(BASE, 72).tobytes() and poses[4].tobytes() == M.pose(BASE, 61).tobytes()
    side.settle()
    against_twin(side, "edits after the change", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 10: launch count
def test_the_launches_do_not_follow_the_number_of_edits():
    side = Side(True)
    side.deform("vertices", "cloth", 14)
    for k in range(60):
        side.add(("s7", "cloth", "cylinder")[k % 3], (GREY, GREEN)[k % 2], 400 + k)
    assert side.change()[3] == 1
    side.add("s7", GREY, 500)
    one = side.change()
    for k in range(30):
        side.remove(5 + k)     # (every second one of the added instances; the base scene's five stay)
    for k in range(10):
        side.add("cloth", GREEN, 510 + k)
        side.rematerial(5 + k, TEXTURED)
    fifty = side.change()
    assert one[3] == fifty[3] == 0 and one[1:3] == (65, 1) and fifty[1:3] == (36, 10), (one, fifty)
    assert one[0] == fifty[0] > 0, (one, fifty)
    against_twin(side, "after fifty edits", emitters=1)


# ---------------------------------------------------------------------------------------------------------------- 11: refusals
def fresh_builder(base=BASE):
    b = M.base_builder(base)
    b.take_origins()
    return b


def raw_change(e, b, origins, n=None, mode=F.TREE_SAH):
    arr = (F.u32 * max(1, len(origins)))(*origins)
    return e.api.raw("change_scene_instances")(e.ctx, b.h if b is not None else None, arr, len(origins) if n is None else n, mode)


def frame_from_nothing(p):
    cam, lights, s = view()
    p.reset_history()
    p.render(cam, s, lights=lights, frame_number=1)
    return snapshot(p)


@pytest.mark.parametrize("state", ["deformed", "device-poses"])
def test_refusals_write_nothing(state):
    side = Side(True)
    e = side.e
    if state == "deformed":
        side.deform("vertices", "cloth", 15)
    else:
        side.device_poses([221, 222, 223, 224, 225])
    reference = frame_from_nothing(side.p)
    report = e.last_instance_change()
    ident = list(range(5))
    zero, nan = np.zeros(16, np.float32), M.pose(BASE, 1).copy()
    nan[5] = np.nan

    def with_new(pose):
        b = fresh_builder()
        b.add_instance(1, GREY, pose)
        return b, ident + [F.INSTANCE_NEW]

    def bad_texture():
        b = fresh_builder()
        m = M.material(BASE, GREY, 0)
        m.base_color_texture = len(side.textures)
        b.add_instance(1, b.add_material(m), M.pose(BASE, 2))
        return b, ident + [F.INSTANCE_NEW]

    def pending_mesh():
        b = fresh_builder()
        M.add_pool_mesh(b, BASE, "s2", "deferred")
        b.finish()
        return b, ident

    def unfinished_mesh():
        b = fresh_builder()
        M.add_pool_mesh(b, BASE, "s2", "host")
        return b, ident

    cases = {
        "ctx NULL": lambda: (e.api.raw("change_scene_instances")(None, side.b.h, (F.u32 * 5)(*ident), 5, F.TREE_SAH), F.HK_E_INVALID),
        "builder NULL": lambda: (raw_change(e, None, ident), F.HK_E_INVALID),
        "origins NULL": lambda: (e.api.raw("change_scene_instances")(e.ctx, side.b.h, None, 5, F.TREE_SAH), F.HK_E_INVALID),
        "tree mode": lambda: (raw_change(e, fresh_builder(), ident, mode=7), F.HK_E_INVALID),
        "n": lambda: (raw_change(e, fresh_builder(), ident, n=4), F.HK_E_INVALID),
        "origin out of range": lambda: (raw_change(e, fresh_builder(), [0, 1, 2, 3, 5]), F.HK_E_INVALID),
        "origin twice": lambda: (raw_change(e, fresh_builder(), [0, 1, 2, 3, 3]), F.HK_E_INVALID),
        "mesh mismatch": lambda: (raw_change(e, fresh_builder(), [0, 2, 1, 3, 4]), F.HK_E_INVALID),
        "singular pose": lambda: (raw_change(e, *with_new(zero)), F.HK_E_INVALID),
        "non-finite pose": lambda: (raw_change(e, *with_new(nan)), F.HK_E_INVALID),
        "texture id": lambda: (raw_change(e, *bad_texture()), F.HK_E_INVALID),
        "deferred mesh": lambda: (raw_change(e, *pending_mesh()), F.HK_E_NOT_READY),
        "unfinished mesh change": lambda: (raw_change(e, *unfinished_mesh()), F.HK_E_NOT_READY),
        "hk_update_scene_instances": lambda: (e.api.raw("update_scene_instances")(e.ctx, side.b.h, F.TREE_SAH), F.HK_E_NOT_READY),
    }
    for name, call in cases.items():
        rc, want = call()
        assert rc == want, (state, name, rc, e.api.last_error())
        assert e.last_instance_change() == report, (state, name, "a refused call changed the report")
        bad = diff_buffers(frame_from_nothing(side.p), reference)
        assert bad == {}, f"{state}, after the refusal '{name}': {bad}"
    assert len(side.materials) == len(side.b.scene().materials)


def test_refusals_without_a_scene_and_of_a_one_slot_scene_changed_on_the_device():
    empty = hk.Engine(device=0)
    assert raw_change(empty, fresh_builder(), list(range(5))) == F.HK_E_NOT_READY
    side = Side(False, base="one_slot")
    reference = frame_from_nothing(side.p)
    side.e.rebuild_trees(F.TREE_SAH)      # (the mirrors are stale from here on)
    after_rebuild = frame_from_nothing(side.p)
    n = len(side.inst)
    side.add("s7", 0, 3)
    assert raw_change(side.e, side.b, list(side.b.origins)) == F.HK_E_NOT_READY, side.e.api.last_error()
    assert diff_buffers(frame_from_nothing(side.p), after_rebuild) == {}
    assert len(side.e.read_instance_transforms(n)) == n and reference.keys() == after_rebuild.keys()


# ---------------------------------------------------------------------------------------------------------------- 12: bands
@MODES
def test_two_bands_change_their_instances_like_the_single_context(threaded):
    from bevy_hikari_amd.distributed import MultiEngine

    flags = F.CTX_DETERMINISTIC_SCATTER
    cam, lights, s = view()
    v, pv = cam.view_uniform(), cam.previous_view_uniform()
    if threaded:
        with product_default_traversal():
            m, ref = MultiEngine([0, 0], flags=flags), hk.Engine(device=0, flags=flags)
    else:
        m, ref = MultiEngine([0, 0], flags=flags), hk.Engine(device=0, flags=flags)
    builders = []
    for e in (m, ref):
        b = M.base_builder(BASE)
        e.upload_noise()
        e.upload_scene(M.scene_of(b, [t["rgba"] for t in M.base_textures()]))
        b.take_origins()
        e.resize(W, H, 1.0)
        builders.append(b)
    m.set_band_bounds([0, 24, H])
    frame = 0
    for step in range(2):
        for e, b in zip((m, ref), builders):
            d = M.pool(BASE, "cylinder")
            idx = b.mesh_index(3)
            if step == 0:
                e.set_mesh_skin(idx, d["positions"], d["normals"], d["joints"], d["weights"])
            e.deform_meshes([("skin", idx, M.joints(3 + step))])
            b.add_instance(3, GREEN, M.pose(BASE, 81 + step))
            b.add_instance(1, GLOW, M.pose(BASE, 91 + step))
            b.remove_instance(0)
            b.set_instance_material(0, GREY)
            e.change_instances(b, F.TREE_SAH)
        for k, c in enumerate(m.contexts):
            assert c.last_instance_change()[1:3] == (4 + step, 2) and not c.last_instance_change()[3] & 2, (k, c.last_instance_change())
            for part, g, w in zip(("records", "alias table"), c.read_emitters(), ref.read_emitters()):
                assert g.tobytes() == w.tobytes(), f"band {k}, step {step}: the emitters' {part} differ from the single context's"
        for _ in range(2):
            frame += 1
            for e in (m, ref):
                e.frame_render(hk.frame_uniform(s, frame), v, pv, lights, s.to_c())
            m.wait(); ref.wait()
            for buf in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_VELOCITY_UV, F.BUF_INSTANCE_MATERIAL, F.BUF_ALBEDO, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
                assert (m.read(buf).view(np.uint8) == ref.read(buf).view(np.uint8)).all(), f"step {step}, frame {frame}: buffer {buf} differs"
