"""Meshes deformed from device memory (hk_deform_meshes_device) with normals recomputed on the device.  The yardstick is a TWIN context
given the same values from numpy through hk_deform_meshes - the recomputed normals from hk_scene_builder_recompute_mesh_normals on a
twin builder: every deformed mesh's geometry, the mesh-level nodes of every ordering, the emitter records with the alias table, both
instance-level trees and one rendered frame must be equal byte for byte.  Frames are 96 x 64 with two bounces.

Shapes: the 17 x 17 grid has 289 vertices (two vertex workgroups, the second of 33) and 512 triangles (two triangle workgroups); the
ribbons end inside a wave (65 triangles) and inside a workgroup (129, 257); the fan's hub sums 40 face vectors; the scene is walked once
from the LDS copy (one ordering) and once beyond it (eight orderings, two slots)."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import deform_items_device
from bevy_hikari_amd.scenes import synthetic_camera
from cases import diff_buffers, product_default_traversal, snapshot
from deform_device_cases import CASES, mesh_of, recomputed_normals

pytestmark = pytest.mark.gpu

SETTINGS = dict(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
RECOMPUTE = dict(recompute_normals=True)


def torch_():
    import torch

    return torch


def build_scene(base):
    """`base` ("small": walked from the LDS copy; "yard": beyond it) plus the meshes of this file, none next to another deformed one:
    grid (recomputed normals) | pad | lamp (emissive; explicit normals) | pad | flag (normals kept) | arm (skinned, 3 joints) | pad |
    fan, zero, hole (the corner cases of the rule).  Returns (scene with .builder, sun, meshes)."""
    if base == "yard":
        scene, sun = S.synthetic_scene(n_boxes=20, n_spheres=5, n_emitters=2, sphere_rings=12, sphere_segs=16)
    else:
        scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    plain = b.add_material(S.standard_material((0.3, 0.6, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (0.6, 1.0, 0.7), 1.0, 0.0, 0.5))
    meshes, slot = {}, [0]

    def place(mesh_id, material):
        k = slot[0]
        slot[0] += 1
        b.add_instance(mesh_id, material, S._trs((-2.4 + 1.2 * (k % 5), 0.3 + 0.1 * k, -1.0 + 1.1 * (k // 5)), (0.0, 0.7 * k, 0.0), (1.0, 1.0, 1.0)))

    def case(name, key):
        c = CASES[key]()
        meshes[name] = dict(id=b.add_mesh(c["positions"], c["normals"], c["uvs"], c["indices"], c["topology"]), rest=c["positions"], normals=c["normals"],
                            moved=c["moved"], kind="recompute")
        place(meshes[name]["id"], plain)

    def ribbon(name, triangles, kind, material=plain):
        p, nr, uv, idx = S.coil_ribbon(triangles)
        m = dict(id=b.add_mesh(p, nr, uv, idx), rest=p, normals=nr, kind=kind)
        if kind == "skin":
            m["joints"], m["weights"] = S.ribbon_skin(p, 3)
        meshes[name] = m
        place(m["id"], material)

    case("grid", "bent_grid")
    ribbon("pad0", 63, None)
    ribbon("lamp", 129, "normals", glow)
    ribbon("pad1", 3, None)
    ribbon("flag", 257, "keep")
    ribbon("arm", 65, "skin")
    ribbon("pad2", 2, None)
    case("fan", "hub_fan")
    case("zero", "zero_area")
    case("hole", "unnamed_vertex")
    scene = b.finish()
    scene.builder = b
    for m in meshes.values():
        m["index"] = b.mesh_index(m["id"])
    return scene, sun, meshes


def pose(m, name, frame):
    """what the mesh's item carries at `frame` (numpy float32): (positions, normals or None) or (joints,)"""
    if m["kind"] == "skin":
        return (S.chain_joints(3, frame, 0.4),)
    if m["kind"] == "recompute":
        w = np.float32(0.4 + 0.3 * frame)
        return (m["rest"] + w * (m["moved"] - m["rest"])).astype(np.float32), None
    q, qn = S.swaying_ribbon(m["rest"], m["normals"], frame, 0.37 * len(name))
    return q, (qn if m["kind"] == "normals" else None)


class Pair:
    """Context A (the device path), context B (hk_deform_meshes from numpy) and a twin BUILDER that mirrors the recomputed normals"""

    def __init__(self, base, default_traversal=False):
        self.plugins, self.scenes, self.meshes = [], [], []
        for _ in range(2):
            scene, self.sun, meshes = build_scene(base)
            if default_traversal:
                with product_default_traversal():
                    p = hk.HikariPlugin(device=0, flags=0)
            else:
                p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
            p.set_scene(scene)
            p.engine.set_mesh_skin(meshes["arm"]["index"], meshes["arm"]["rest"], meshes["arm"]["normals"], meshes["arm"]["joints"], meshes["arm"]["weights"])
            self.plugins.append(p); self.scenes.append(scene); self.meshes.append(meshes)
        self.a, self.b = self.plugins
        self.ma, self.mb = self.meshes
        self.mirror_scene, _, self.mm = build_scene(base)
        self.mirror = self.mirror_scene.builder
        self.cam, self.lights, self.settings = synthetic_camera(96, 64), hk.lights_uniform(directional=self.sun), hk.HikariSettings(**SETTINGS)
        self.device = torch_().device("cuda", 0)

    def mirrored_normals(self, name, positions):
        """hk_scene_builder_set_mesh_vertices(positions, NULL) + hk_scene_builder_recompute_mesh_normals on the twin builder"""
        m = self.mm[name]
        self.mirror.set_mesh_vertices(m["id"], positions)
        self.mirror.recompute_mesh_normals(m["id"])
        scene = self.mirror.finish()
        return mesh_of(scene, self.mirror.mesh_index(m["id"]), len(positions))[1]

    def items(self, names, frame, strided=("grid",)):
        """(torch items for A, numpy items for B) of the named meshes at `frame`"""
        torch = torch_()
        ta, tb = [], []
        for name in names:
            ma, mb = self.ma[name], self.mb[name]
            values = pose(ma, name, frame)
            if ma["kind"] == "skin":
                ta.append(("skin", ma["index"], torch.from_numpy(values[0]).to(self.device)))
                tb.append(("skin", mb["index"], values[0]))
                continue
            q, qn = values
            if name in strided:   # a column slice of a wider state tensor: 32 bytes from row to row, 40 bytes into its storage
                state = torch.full((len(q) + 1, 8), 7.5, dtype=torch.float32, device=self.device)
                state[1:, 2:5] = torch.from_numpy(q).to(self.device)
                tq = state[1:, 2:5]
                assert tq.stride(0) == 8 and tq.storage_offset() == 10
            else:
                tq = torch.from_numpy(q).to(self.device)
            if ma["kind"] == "recompute":
                ta.append(("vertices", ma["index"], tq, None, RECOMPUTE))
                tb.append(("vertices", mb["index"], q, self.mirrored_normals(name, q)))
            else:
                ta.append(("vertices", ma["index"], tq, None if qn is None else torch.from_numpy(qn).to(self.device)))
                tb.append(("vertices", mb["index"], q, qn))
        return ta, tb

    def deform(self, names, frame, **kw):
        ta, tb = self.items(names, frame, **kw)
        self.a.engine.deform_meshes(ta)
        self.b.engine.deform_meshes(tb)

    def render(self, n):
        for p in self.plugins:
            p.render(self.cam, self.settings, lights=self.lights, frame_number=n)

    def assert_same(self, names, what, frame=True):
        a, b = self.a.engine, self.b.engine
        na, ca, oa = a.read_mesh_nodes()
        nb, cb, ob = b.read_mesh_nodes()
        assert (ca, oa) == (cb, ob) and bytes(na) == bytes(nb), f"{what}: mesh-level nodes differ"
        (ra, aa), (rb, ab) = a.read_emitters(), b.read_emitters()
        assert ra.tobytes() == rb.tobytes() and aa.tobytes() == ab.tobytes(), f"{what}: emitter records / alias tables differ"
        counts = len(self.scenes[0].instance_nodes), len(self.scenes[0].emissive_nodes)
        for x, y in zip(a.read_trees(*counts), b.read_trees(*counts)):
            assert bytes(x) == bytes(y), f"{what}: instance-level trees differ"
        for name in names:
            ga, gb = a.read_mesh_geometry(self.ma[name]["index"]), b.read_mesh_geometry(self.mb[name]["index"])
            for key in ("positions", "normals", "triangles", "box"):
                assert ga[key].tobytes() == gb[key].tobytes(), f"{what}: {key} of mesh {name} differ"
        if frame:
            bad = diff_buffers(snapshot(self.a), snapshot(self.b))
            assert bad == {}, f"{what}: {bad}"


def restated(pair, name, positions, current):
    """the numpy float32 restatement of the rule for mesh `name` of context A's scene"""
    m = pair.ma[name]
    tris = mesh_of(pair.scenes[0], m["index"], len(m["rest"]))[2]
    return recomputed_normals(positions, tris, current)


EVERYTHING = ["grid", "lamp", "flag", "arm"]


# ---- 1
@pytest.mark.parametrize("base,default_traversal", [("small", False), ("yard", True)], ids=["lds_copy", "eight_orderings"])
def test_one_batch_with_everything(base, default_traversal):
    pair = Pair(base, default_traversal)
    pair.render(1)
    mode, orderings = C.c_uint32(), C.c_uint32()
    pair.a.engine.api.call("traversal_mode", pair.a.engine.ctx, C.byref(mode), C.byref(orderings))
    assert orderings.value == (8 if default_traversal else 1)
    pair.deform(EVERYTHING, 2)
    assert pair.a.engine.last_deform()[:4] == (4, 289 + 131 + 259 + 67, 512 + 129 + 257 + 65, 6)
    pair.render(2)
    pair.assert_same(EVERYTHING, "one batch with everything")
    geo = pair.a.engine.read_mesh_geometry(pair.ma["grid"]["index"])
    q = pose(pair.ma["grid"], "grid", 2)[0]
    want, kept = restated(pair, "grid", q, pair.ma["grid"]["normals"])
    assert geo["positions"][:, :3].tobytes() == q.tobytes() and not kept.any()
    assert np.ascontiguousarray(geo["normals"][:, :3]).tobytes() == want.tobytes(), "the device normals differ from the float32 restatement"
    # what the host may still upload: the flags a host-path batch leaves
    answers = [p.engine.api.raw("upload_scene_instances")(p.engine.ctx, s.builder.h) for p, s in zip(pair.plugins, pair.scenes)]
    assert answers == [F.HK_E_NOT_READY, F.HK_E_NOT_READY]


# ---- 2
def test_six_launches_with_a_flagged_item_five_without_and_two_runs_are_equal():
    runs = []
    for _ in range(2):
        pair = Pair("small")
        pair.render(1)
        ta, _ = pair.items(["lamp", "flag", "arm"], 2)
        pair.a.engine.deform_meshes(ta)
        assert pair.a.engine.last_deform()[:4] == (3, 131 + 259 + 67, 129 + 257 + 65, 5)
        ta, _ = pair.items(["grid", "fan", "arm"], 3)
        pair.a.engine.deform_meshes(ta)
        assert pair.a.engine.last_deform()[:4] == (3, 289 + 41 + 67, 512 + 40 + 65, 6)
        pair.a.render(pair.cam, pair.settings, lights=pair.lights, frame_number=2)
        geo = {n: pair.a.engine.read_mesh_geometry(pair.ma[n]["index"]) for n in ("grid", "fan", "lamp", "flag", "arm")}
        runs.append((snapshot(pair.a), {n: {k: v.tobytes() for k, v in g.items()} for n, g in geo.items()}))
    assert diff_buffers(runs[0][0], runs[1][0]) == {}
    assert runs[0][1] == runs[1][1]


# ---- 3
def test_hub_fan_zero_area_triangle_and_unnamed_vertex_on_the_device():
    pair = Pair("small")
    names = ["fan", "zero", "hole"]
    pair.deform(names, 2, strided=("fan",))
    pair.render(1)
    pair.assert_same(names, "corner cases")
    for name in names:
        m = pair.ma[name]
        geo = pair.a.engine.read_mesh_geometry(m["index"])
        want, kept = restated(pair, name, pose(m, name, 2)[0], m["normals"])
        got = np.ascontiguousarray(geo["normals"][:, :3])
        assert got.tobytes() == want.tobytes(), name
        assert got[kept].tobytes() == m["normals"][kept].tobytes()   # an all-zero sum keeps the normal there was
    assert list(np.flatnonzero(restated(pair, "zero", pose(pair.ma["zero"], "zero", 2)[0], pair.ma["zero"]["normals"])[1])) == [5]
    assert list(np.flatnonzero(restated(pair, "hole", pose(pair.ma["hole"], "hole", 2)[0], pair.ma["hole"]["normals"])[1])) == [2]


# ---- 4
def test_the_producer_stream_is_ordered_before_and_after_the_call():
    torch = torch_()
    pair = Pair("small")
    pair.render(1)
    m = pair.ma["grid"]
    first, second = pose(m, "grid", 2)[0], pose(m, "grid", 5)[0]
    half = torch.from_numpy(first * np.float32(0.5)).to(pair.device)   # (x 2 on the device is exact: B is given `first` itself)
    other = torch.from_numpy(second).to(pair.device)
    busy = torch.randn((2048, 2048), device=pair.device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(pair.device)
    with torch.cuda.stream(stream):
        for _ in range(8):                       # the producing kernel is queued behind work that takes a while
            busy = torch.mm(busy, busy) * 1e-3
        positions = half * 2.0
        pair.a.engine.deform_meshes([("vertices", m["index"], positions, None, RECOMPUTE)], producer_stream=stream)
        positions.copy_(other)                   # overwritten in stream order right after the call
    pair.b.engine.deform_meshes([("vertices", pair.mb["grid"]["index"], first, pair.mirrored_normals("grid", first))])
    pair.render(2)
    pair.assert_same(["grid"], "positions produced on a side stream")
    with torch.cuda.stream(stream):
        pair.a.engine.deform_meshes([("vertices", m["index"], positions, None, RECOMPUTE)], producer_stream=stream)
        positions.zero_()
    pair.b.engine.deform_meshes([("vertices", pair.mb["grid"]["index"], second, pair.mirrored_normals("grid", second))])
    pair.render(3)
    pair.assert_same(["grid"], "the overwritten tensor")
    stream.synchronize()


# ---- 5
def test_refused_batches_write_nothing():
    torch = torch_()
    pair = Pair("small")
    api, ctx = pair.a.engine.api, pair.a.engine.ctx
    before = pair.a.engine.last_deform()
    good, _ = pair.items(["lamp", "grid", "arm"], 2, strided=())
    host = np.zeros((289, 3), np.float32)
    two = torch.from_numpy(S.chain_joints(2, 2)).to(pair.device)
    idx = pair.ma["grid"]["index"]
    unknown = F.HkMeshIndex(idx.vertex, idx.primitive, idx.node_offset + 1, idx.node_count)
    grid_normals = torch.zeros((289, 3), device=pair.device)

    def swap(item):
        return [good[0], item, good[2]]

    cases = {
        "a pageable host pointer": (good, lambda t: setattr(t[1], "data", host.ctypes.data)),
        "pageable host normals": (swap(("vertices", idx, good[1][2], grid_normals)), lambda t: setattr(t[1], "normals", host.ctypes.data)),
        "a misaligned pointer": (good, lambda t: setattr(t[1], "data", t[1].data + 2)),
        "a misaligned palette": ([good[0], ("skin", pair.ma["arm"]["index"], good[2][2]), good[1]], lambda t: setattr(t[1], "data", t[1].data + 4)),
        "a stride of 8": (good, lambda t: setattr(t[1], "data_stride", 8)),
        "a stride of 14": (good, lambda t: setattr(t[1], "data_stride", 14)),
        "a palette stride": ([good[0], ("skin", pair.ma["arm"]["index"], good[2][2]), good[1]], lambda t: setattr(t[1], "data_stride", 128)),
        "an unknown flag bit": (good, lambda t: setattr(t[1], "flags", 3)),
        "recompute with normals": (swap(("vertices", idx, good[1][2], grid_normals)), lambda t: setattr(t[1], "flags", F.DEFORM_RECOMPUTE_NORMALS)),
        "recompute on a skin item": ([good[0], ("skin", pair.ma["arm"]["index"], good[2][2]), good[1]], lambda t: setattr(t[1], "flags", F.DEFORM_RECOMPUTE_NORMALS)),
        "a mesh named twice": (swap(good[0]), None),
        "an unknown mesh record": (swap(("vertices", unknown, good[1][2], None)), None),
        "n_joints at or below the skin's highest joint": ([good[0], ("skin", pair.ma["arm"]["index"], two), good[1]], None),
    }
    assert int(pair.ma["arm"]["joints"].max()) == 2
    for what, (items, patch) in cases.items():
        assert len(items) == 3
        table, keep = deform_items_device(items, 0)
        if patch:
            patch(table)
        rc = api.raw("deform_meshes_device")(ctx, table, 3, None)
        message = api.last_error()
        assert rc == F.HK_E_INVALID, (what, rc, message)
        assert "item 1" in message, (what, message)
    assert api.raw("deform_meshes_device")(ctx, None, 0, None) == F.HK_OK   # n == 0: nothing to do
    assert pair.a.engine.last_deform() == before
    torch.cuda.synchronize()
    pair.render(1)
    pair.assert_same(["grid", "lamp", "arm"], "after the refusals")   # B made no call at all
    assert api.raw("upload_scene_instances")(ctx, pair.scenes[0].builder.h) == F.HK_OK   # nothing is stale: nothing was deformed


# ---- 6
def test_later_calls_behave_as_after_the_host_path():
    pair = Pair("yard", default_traversal=True)
    pair.render(1)
    pair.deform(EVERYTHING, 2)
    for p, meshes in zip(pair.plugins, pair.meshes):
        p.engine.rebuild_mesh_tree(meshes["grid"]["index"], F.TREE_SAH)
    pair.render(2)
    pair.assert_same(EVERYTHING, "mesh tree rebuild after the device path")
    mover = len(pair.scenes[0].instances) - 3
    for p, scene in zip(pair.plugins, pair.scenes):
        moved = np.ctypeslib.as_array(scene.instances[mover].model).copy()
        moved[12] += 0.2
        scene.builder.set_instance_transform(mover, moved)
        assert p.engine.refit_instances(scene.builder) == 1
    pair.deform(EVERYTHING, 3)                 # the new topology is refit
    pair.render(3)
    pair.assert_same(EVERYTHING, "instance refit + a second device batch")
    for p, meshes in zip(pair.plugins, pair.meshes):   # ... and the HOST path on both, over what the device path left
        q = pose(meshes["grid"], "grid", 4)[0]
        p.engine.deform_meshes([("vertices", meshes["grid"]["index"], q, None), ("skin", meshes["arm"]["index"], S.chain_joints(3, 4, 0.4)),
                                ("vertices", meshes["flag"]["index"]) + pose(meshes["flag"], "flag", 4)])
        assert p.engine.last_deform()[3] == 5
    pair.render(4)
    pair.assert_same(EVERYTHING, "a host-path batch of the same meshes")


# ---- 7
def test_engine_routes_torch_items_to_the_device_path_and_numpy_items_to_the_old_one():
    pair = Pair("small")
    ta, tb = pair.items(["grid", "arm"], 2)
    pair.a.engine.deform_meshes(ta)                                   # torch's current (default) stream stands for the producer
    assert pair.a.engine.last_deform()[:4] == (2, 289 + 67, 512 + 65, 6)   # six launches: only hk_deform_meshes_device has the normals launch
    pair.b.engine.deform_meshes(tb)
    assert pair.b.engine.last_deform()[:4] == (2, 289 + 67, 512 + 65, 5)
    pair.render(1)
    pair.assert_same(["grid", "arm"], "routed by the items' arrays")
    q = pose(pair.mb["grid"], "grid", 3)[0]
    with pytest.raises(ValueError):
        pair.b.engine.deform_meshes([("vertices", pair.mb["grid"]["index"], q, None, RECOMPUTE)])           # the host path has no such flag
    with pytest.raises(ValueError):
        pair.a.engine.deform_meshes([ta[0], ("skin", pair.ma["arm"]["index"], S.chain_joints(3, 3))])      # one batch, one kind of memory
