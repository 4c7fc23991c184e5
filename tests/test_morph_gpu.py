"""Morph targets blended on the device (HK_DEFORM_MORPH / HK_DEFORM_MORPH_SKIN items of hk_deform_meshes and hk_deform_meshes_device).  The
yardstick of every comparison is a TWIN context that is given scenes.morph_reference's vertices - a numpy float32 restatement of the
contract - through the parent's calls: hk_update_mesh_vertices for a morph item, hk_set_mesh_skin(the morphed bind pose) + hk_skin_mesh
for a morph + skin item.  Every screen buffer, the mesh-level nodes of every ordering, the emitter records with the alias table, every
mesh's positions, normals, triangles and box, and the staleness answers must be equal bit for bit.  Frames are 96 x 64 with two bounces.

Shapes, the smallest at which the kernels can go wrong: meshes of 1, 2, 63, 65, 257 and 722 triangles (vertex counts that end inside a
wave and inside a workgroup), sets of 1, 63, 65, 257 and 300 targets (the active list crosses a wave and the 256 threads of the begin
workgroup), active counts of 0, 1, all and every other one, sets with and without normal deltas, more than 64 items in one batch."""
import ctypes as C

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.plugin import deform_items, deform_items_device
from test_deform_batch_gpu import assert_same_frame, assert_same_scene, assert_same_staleness, frame_tools, plugin

pytestmark = pytest.mark.gpu

MODES = ["wave", "none", "all", "one", "alternate"]
# (triangles, targets, kind, normal deltas, joints, flags): "e" = an emitter, "2" = a second instance
MAIN = [(1, 1, "morph", True, 0, ""), (2, 63, "morph", False, 0, ""), (63, 65, "morph_skin", True, 3, ""), (65, 257, "morph", True, 0, "e2"),
        (257, 300, "morph_skin", False, 17, ""), (722, 300, "morph", True, 0, ""), (65, 63, "morph", False, 0, "2"), (257, 65, "morph", True, 0, ""),
        (722, 1, "morph_skin", True, 1, ""), (63, 0, "vertices", True, 0, ""), (65, 0, "skin", True, 3, ""), (2, 257, "morph_skin", True, 1, "")]
SMALL = [(3, 65, "morph", True, 0, "e2"), (65, 300, "morph_skin", True, 3, ""), (257, 63, "morph", False, 0, ""), (64, 0, "skin", True, 3, ""), (128, 1, "morph", True, 0, "")]
MIXED = [((2, 3, 63, 65, 64)[k % 5], (1, 3, 65, 5)[k % 4] if k % 4 != 3 else 0, ("morph", "morph_skin", "morph", "vertices" if k % 8 == 3 else "skin")[k % 4], k % 3 != 0,
          (0, 3, 0, 3)[k % 4], "") for k in range(70)]


def build_scene(base, specs):
    """`base` ("yard" / "small", as scenes.crowd_scene) plus one coil_ribbon per spec.  Returns (scene with .builder, sun, meshes): meshes maps
    "m0", "m1", ... to dict(id, index, rest, normals, kind, dp, dn, joints, weights (of the skin), nj, phase)."""
    if base == "yard":
        scene, sun = S.synthetic_scene(n_boxes=20, n_spheres=5, n_emitters=2, sphere_rings=12, sphere_segs=16)
    else:
        scene, sun = S.synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    plain = b.add_material(S.standard_material((0.3, 0.6, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
    glow = b.add_material(S.standard_material((0.9, 0.9, 0.9, 1.0), (0.6, 1.0, 0.7), 1.0, 0.0, 0.5))
    side = max(int(np.ceil(np.sqrt(len(specs)))), 1)
    meshes = {}
    for k, (triangles, targets, kind, normal_deltas, nj, flags) in enumerate(specs):
        p, nr, uv, idx = S.coil_ribbon(triangles)
        m = dict(id=b.add_mesh(p, nr, uv, idx), rest=p, normals=nr, kind=kind, nj=nj, phase=0.37 * k, k=k, targets=targets)
        if targets:
            m["dp"], m["dn"] = S.morph_targets(p, nr, targets, seed=k, normal_deltas=normal_deltas)
        if nj:
            m["joints"], m["weights"] = S.ribbon_skin(p, nj)
        x, z = ((k % side + 0.5) / side - 0.5) * 6.4, ((k // side + 0.5) / side - 0.5) * 6.4
        b.add_instance(m["id"], glow if "e" in flags else plain, S._trs((x, 0.05, z), (0.0, 0.9 * k, 0.0), (1.0, 1.0, 1.0)))
        if "2" in flags:
            b.add_instance(m["id"], glow if "e" in flags else plain, S._trs((x + 0.3, 1.3, z - 0.2), (0.3, 0.5 * k, 0.1), (0.7, 0.8, 0.7)))
        meshes[f"m{k}"] = m
    scene = b.finish()
    scene.builder = b
    for m in meshes.values():
        m["index"] = b.mesh_index(m["id"])
    return scene, sun, meshes


def set_up(engine, meshes, morph=True):
    """what a host does once per mesh: the skin (its bind planes are what a plain skin item reads) and the morph set (not the twin's)"""
    for m in meshes.values():
        if m["nj"]:
            engine.set_mesh_skin(m["index"], m["rest"], m["normals"], m["joints"], m["weights"])
        if m["targets"] and morph:
            engine.set_mesh_morph_targets(m["index"], m["rest"], m["normals"], m["dp"], m["dn"])


def mode_of(m, frame):
    return MODES[(m["k"] + frame) % len(MODES)]


def weights_of(m, frame):
    return S.morph_weights(m["targets"], frame, m["phase"], mode_of(m, frame))


def items_of(meshes, frame, names=None):
    """the batch of the context under test at `frame`"""
    out = []
    for name in names or meshes:
        m = meshes[name]
        if m["kind"] == "morph":
            out.append(("morph", m["index"], weights_of(m, frame)))
        elif m["kind"] == "morph_skin":
            out.append(("morph_skin", m["index"], S.chain_joints(m["nj"], frame, m["phase"]), weights_of(m, frame)))
        elif m["kind"] == "skin":
            out.append(("skin", m["index"], S.chain_joints(m["nj"], frame, m["phase"])))
        else:
            q, qn = S.swaying_ribbon(m["rest"], m["normals"], frame, m["phase"])
            out.append(("vertices", m["index"], q, qn if m["k"] % 2 else None))
    return out


def twin_calls(engine, meshes, items, names=None):
    """the yardstick: the parent's single-mesh calls on the morphed vertices of the numpy restatement, in item order"""
    for name, item in zip(names or meshes, items):
        m = meshes[name]
        if item[0] == "morph":
            q, qn = S.morph_reference(m["rest"], m["normals"], m["dp"], m["dn"], item[2])
            engine.update_mesh_vertices(m["index"], q, qn)
        elif item[0] == "morph_skin":
            q, qn = S.morph_reference(m["rest"], m["normals"], m["dp"], m["dn"], item[3])
            engine.set_mesh_skin(m["index"], q, qn, m["joints"], m["weights"])
            engine.skin_mesh(m["index"], item[2])
        elif item[0] == "skin":
            engine.skin_mesh(m["index"], item[2])
        else:
            engine.update_mesh_vertices(m["index"], item[2], item[3])


def make_pair(base, specs, flags=F.CTX_DETERMINISTIC_SCATTER, default_traversal=False):
    out = []
    for which in range(2):
        scene, sun, meshes = build_scene(base, specs)
        p = plugin(flags, default_traversal)
        p.set_scene(scene)
        set_up(p.engine, meshes, morph=which == 0)
        out.append((p, scene, meshes))
    return out[0], out[1], sun


def run_sequence(base, specs, frames, default_traversal=False, deform_before_first=False):
    (gpu, gs, gm), (twin, ts, tm), sun = make_pair(base, specs, 0 if default_traversal else F.CTX_DETERMINISTIC_SCATTER, default_traversal)
    cam, lights, s = frame_tools(sun)
    moved = {name: False for name in gm}
    some_zero = all_zero = False
    for n in range(1, frames + 1):
        if n > 1 or deform_before_first:
            items = items_of(gm, n + 1)
            for m in gm.values():
                if m["targets"]:
                    w = weights_of(m, n + 1)
                    some_zero |= bool((w == 0).any() and (w != 0).any())
                    all_zero |= bool((w == 0).all())
            gpu.engine.deform_meshes(items)
            assert gpu.engine.last_deform()[0] == len(items) and gpu.engine.last_deform()[3] == 5   # begin, vertices, triangles, boxes, emit
            twin_calls(twin.engine, tm, items_of(tm, n + 1))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        assert_same_frame(gpu, twin, f"frame {n}")
        assert_same_scene(gpu, twin, gm, tm, f"frame {n}")
        stale = assert_same_staleness(gpu, gs, twin, ts, f"frame {n}")
        if n > 1 or deform_before_first:
            assert stale[:2] == (F.HK_E_NOT_READY, F.HK_E_NOT_READY)   # (the host mirrors no longer describe the meshes)
        for name, m in gm.items():
            moved[name] |= not np.array_equal(gpu.engine.read_mesh_geometry(m["index"])["positions"][:, :3], m["rest"])
    assert all(moved.values()), f"the poses must move every mesh: {moved}"
    return gpu, twin, some_zero, all_zero


# ---- 1
@pytest.mark.parametrize("default_traversal", [False, True], ids=["reference_walk", "product_default"])
def test_morphing_crowd_equals_the_twin_given_the_restatement(default_traversal):
    """12 meshes of 1 .. 722 triangles with sets of 1 .. 300 targets, morph and morph + skin items (palettes of 1, 3, 17 joints) beside a
    vertex item and a skin item, one morphing emitter with two instances; the weights' mode turns from frame to frame (some zero, all
    zero, none zero, one, every other one).  Once with the suite's flags, once with the product default (eight orderings, wide records)."""
    assert {t for t, *_ in MAIN} >= {1, 2, 63, 65, 257, 722} and {n for _, n, *_ in MAIN} >= {1, 63, 65, 257, 300}
    gpu, _, some_zero, all_zero = run_sequence("yard", MAIN, 4, default_traversal=default_traversal)
    assert some_zero and all_zero, "a frame with a weight of exactly zero and one with all weights zero are part of the sequence"
    if default_traversal:
        mode, orderings = C.c_uint32(), C.c_uint32()
        gpu.engine.api.call("traversal_mode", gpu.engine.ctx, C.byref(mode), C.byref(orderings))
        assert orderings.value == 8 and mode.value & F.TRAVERSAL_WIDE


# ---- 2
def test_small_scene_from_the_lds_copy():
    """The small base (LDS scene, one slot), 5 meshes, 4 frames."""
    _, _, some_zero, all_zero = run_sequence("small", SMALL, 4)
    assert some_zero and all_zero


# ---- 3
def test_seventy_items_of_four_kinds_in_one_batch():
    """More items than a wave has lanes: vertices, skin, morph and morph + skin items in one batch, two batches."""
    kinds = [k for _, _, k, *_ in MIXED]
    assert len(MIXED) > 64 and all(kinds.count(k) >= 8 for k in ("vertices", "skin", "morph", "morph_skin"))
    run_sequence("yard", MIXED, 2, deform_before_first=True)


# ---- 4
def test_every_active_count_against_the_host_twin():
    """One mesh of 257 triangles and 300 targets (with normal deltas), weights with 0, 1, 150 (every other one), 299 and 300 active targets, the
    last ones straddling the 256 of the begin workgroup: positions and normals equal hk_morph_vertices' bytes."""
    scene, sun, meshes = build_scene("small", [(257, 300, "morph", True, 0, "")])
    p = plugin()
    p.set_scene(scene)
    set_up(p.engine, meshes)
    m = meshes["m0"]
    cases = {mode: S.morph_weights(300, 3, 0.1, mode) for mode in ("none", "one", "alternate", "all")}
    cases["all but 255"] = cases["all"].copy()
    cases["all but 255"][255] = -0.0
    cases["255, 256 and 299"] = np.zeros(300, np.float32)
    cases["255, 256 and 299"][[255, 256, 299]] = [0.5, -1.25, 2.0]
    for what, w in cases.items():
        p.engine.deform_meshes([("morph", m["index"], w)])
        geo = p.engine.read_mesh_geometry(m["index"])
        want = hk.morph_vertices(m["rest"], m["normals"], m["dp"], m["dn"], w)
        assert np.ascontiguousarray(geo["positions"][:, :3]).tobytes() == want[0].tobytes(), what
        assert np.ascontiguousarray(geo["normals"][:, :3]).tobytes() == want[1].tobytes(), what


# ---- 5
def test_device_sources_and_the_producer_stream():
    """The same items from torch tensors: the weights of one item produced on a side stream behind a long queue and overwritten right after
    the call, the weights of another a slice at a non-zero offset of a larger tensor."""
    import torch

    (gpu, gs, gm), (twin, ts, tm), sun = make_pair("small", SMALL)
    cam, lights, s = frame_tools(sun)
    device = torch.device("cuda", 0)
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)
    host_items = items_of(gm, 2)
    busy = torch.zeros((1 << 26,), device=device)
    pool = torch.full((1024,), 7.5, dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device)
    with torch.cuda.stream(stream):
        for _ in range(32):                      # the producing kernels are queued behind work that takes a while
            busy.add_(1.0)
        items, tensors = [], []
        for k, item in enumerate(host_items):
            arrays = []
            for a in item[2:]:
                if a is None:
                    arrays.append(None)
                elif a.ndim == 1 and k == 1:     # the weights of the morph + skin item: a slice 37 floats into a larger tensor
                    pool[37:37 + len(a)] = torch.from_numpy(a).to(device)
                    arrays.append(pool[37:37 + len(a)])
                    assert arrays[-1].storage_offset() == 37
                else:
                    arrays.append(torch.from_numpy(a * np.float32(0.5)).to(device) * 2.0)   # (x 2 on the device is exact)
            tensors += [a for a in arrays if a is not None]
            items.append(item[:2] + tuple(arrays))
        assert items[1][0] == "morph_skin" and items[0][0] == "morph"
        gpu.engine.deform_meshes(items, producer_stream=stream)
        for t in tensors:                        # overwritten in stream order right after the call
            t.fill_(3.0)
    assert gpu.engine.last_deform()[:4] == (len(items), sum(len(m["rest"]) for m in gm.values()), sum(t for t, *_ in SMALL), 5)
    twin_calls(twin.engine, tm, items_of(tm, 2))
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=2)
    assert_same_frame(gpu, twin, "weights produced on a side stream")
    assert_same_scene(gpu, twin, gm, tm, "weights produced on a side stream")
    assert_same_staleness(gpu, gs, twin, ts, "after the device path")
    stream.synchronize()
    with pytest.raises(ValueError):              # one batch, one kind of memory
        gpu.engine.deform_meshes([items[0], host_items[2]])


def scene_bytes(p, meshes):
    nodes = bytes(p.engine.read_mesh_nodes()[0])
    records, alias = p.engine.read_emitters()
    geo = [p.engine.read_mesh_geometry(m["index"]) for m in meshes.values()]
    return nodes, records.tobytes(), alias.tobytes(), [{k: v.tobytes() for k, v in g.items()} for g in geo]


# ---- 6
def test_refused_device_sources_write_nothing():
    import torch

    scene, sun, meshes = build_scene("small", SMALL)
    p = plugin()
    p.set_scene(scene)
    set_up(p.engine, meshes)
    api, ctx = p.engine.api, p.engine.ctx
    p.engine.deform_meshes(items_of(meshes, 2))
    before, counts = scene_bytes(p, meshes), p.engine.last_deform()
    device = torch.device("cuda", 0)
    good = [item[:2] + tuple(torch.from_numpy(a).to(device) for a in item[2:]) for item in items_of(meshes, 3)[:3]]
    assert [g[0] for g in good] == ["morph", "morph_skin", "morph"]
    host = np.zeros(512, np.float32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
    block, size = C.c_void_p(), 1 << 21
    assert hip.hipMalloc(C.byref(block), size) == 0
    swapped = [good[1], good[0], good[2]]        # item 1: the plain morph item (65 weights)
    cases = {
        "pageable weights (morph + skin)": (good, lambda t: setattr(t[1], "normals", host.ctypes.data)),
        "pageable weights (morph)": (swapped, lambda t: setattr(t[1], "data", host.ctypes.data)),
        "misaligned weights (morph + skin)": (good, lambda t: setattr(t[1], "normals", t[1].normals + 2)),
        "misaligned weights (morph)": (swapped, lambda t: setattr(t[1], "data", t[1].data + 2)),
        "weights one float short of their allocation (morph + skin)": (good, lambda t: setattr(t[1], "normals", block.value + size - 4 * 299)),
        "weights one float short of their allocation (morph)": (swapped, lambda t: setattr(t[1], "data", block.value + size - 4 * 64)),
        "a weights stride of 8 (morph)": (swapped, lambda t: setattr(t[1], "data_stride", 8)),
        "a weights stride of 8 (morph + skin)": (good, lambda t: setattr(t[1], "normals_stride", 8)),
        "a palette stride (morph + skin)": (good, lambda t: setattr(t[1], "data_stride", 128)),
        "a misaligned palette (morph + skin)": (good, lambda t: setattr(t[1], "data", t[1].data + 4)),
        "recompute on a morph item": (swapped, lambda t: setattr(t[1], "flags", F.DEFORM_RECOMPUTE_NORMALS)),
        "recompute on a morph + skin item": (good, lambda t: setattr(t[1], "flags", F.DEFORM_RECOMPUTE_NORMALS)),
        "an unknown flag bit": (good, lambda t: setattr(t[1], "flags", 3)),
        "an unknown kind": (good, lambda t: setattr(t[1], "kind", 7)),
    }
    assert meshes["m1"]["targets"] == 300 and meshes["m0"]["targets"] == 65
    for what, (items, patch) in cases.items():
        table, keep = deform_items_device(items, 0)
        patch(table)
        rc = api.raw("deform_meshes_device")(ctx, table, 3, None)
        message = api.last_error()
        assert rc == F.HK_E_INVALID, (what, rc, message)
        assert "item 1" in message, (what, message)
    # a stride of 4 is the packed one
    table, keep = deform_items_device(good, 0)
    table[0].data_stride, table[1].normals_stride, table[1].data_stride = 4, 4, 64
    assert p.engine.last_deform() == counts
    torch.cuda.synchronize()
    assert scene_bytes(p, meshes) == before, "a refused batch wrote to the scene"
    assert api.raw("deform_meshes_device")(ctx, table, 3, None) == F.HK_OK
    assert hip.hipFree(block) == 0
    for name, item in zip(meshes, items_of(meshes, 3)[:3]):
        m = meshes[name]
        want = S.morph_reference(m["rest"], m["normals"], m["dp"], m["dn"], item[-1])
        if item[0] == "morph":
            assert np.ascontiguousarray(p.engine.read_mesh_geometry(m["index"])["positions"][:, :3]).tobytes() == want[0].tobytes(), name


# ---- 7
def test_refusal_table_of_the_host_path_and_five_launches():
    """Every entry of the validation list that a caller can produce, as item 6 of a batch of 8; each leaves the scene's bytes untouched.  Kind 7
    is still refused, and so is a mesh named twice."""
    specs = [(65, 5, "morph", True, 0, ""), (63, 3, "morph_skin", True, 3, ""), (2, 1, "morph", False, 0, ""), (64, 0, "skin", True, 3, ""), (3, 0, "vertices", True, 0, ""),
             (65, 2, "morph", True, 0, ""), (63, 4, "morph_skin", True, 3, ""), (65, 7, "morph", True, 0, ""),
             (63, 0, "skin", True, 3, ""), (65, 0, "vertices", True, 0, ""), (64, 3, "morph", True, 17, ""), (63, 2, "morph", True, 0, "")]
    scene, sun, meshes = build_scene("small", specs)
    p = plugin()
    p.set_scene(scene)
    set_up(p.engine, meshes)
    api, ctx = p.engine.api, p.engine.ctx
    names = list(meshes)
    good = items_of(meshes, 2, names[:8])
    p.engine.deform_meshes(good)
    assert p.engine.last_deform()[:4] == (8, sum(len(meshes[n]["rest"]) for n in names[:8]), sum(t for t, *_ in specs[:8]), 5)
    before = scene_bytes(p, meshes)
    m6, skin_only, plain, other_count, morph_only = (meshes[names[k]] for k in (6, 8, 9, 10, 11))
    # (a skin and a morph set of differing vertex counts cannot be made: both set calls accept the mesh's own vertex count alone)
    identity = lambda n: np.tile(np.eye(4, dtype=np.float32).reshape(-1), (n, 1))
    swap = lambda item: good[:6] + [item] + good[7:]
    w4 = weights_of(m6, 2)
    cases = {
        "morph without a set": (swap(("morph", plain["index"], np.ones(3, np.float32))), None),
        "morph + skin without a morph set": (swap(("morph_skin", skin_only["index"], identity(3), np.ones(3, np.float32))), None),
        "morph + skin without a skin": (swap(("morph_skin", morph_only["index"], identity(3), np.ones(2, np.float32))), None),
        "count below the set's target count": (swap(("morph", morph_only["index"], np.ones(1, np.float32))), None),
        "count above the set's target count": (swap(("morph", morph_only["index"], np.ones(3, np.float32))), None),
        "morph with normals": (good, lambda t: (setattr(t[6], "kind", F.DEFORM_MORPH), setattr(t[6], "count", 4), setattr(t[6], "data", t[6].normals))),
        "morph + skin with NULL weights": (good, lambda t: setattr(t[6], "normals", None)),
        "a joint index at or above count": (swap(("morph_skin", other_count["index"], identity(3), np.ones(3, np.float32))), None),
        "NULL data": (good, lambda t: setattr(t[6], "data", None)),
        "unknown kind": (good, lambda t: setattr(t[6], "kind", 7)),
        "a mesh named twice": (swap(good[2]), None),
    }
    assert int(other_count["joints"].max()) == 16 and len(w4) == 4
    for what, (items, patch) in cases.items():
        assert len(items) == 8
        table, keep = deform_items(items)
        if patch:
            patch(table)
        rc = api.raw("deform_meshes")(ctx, table, len(items))
        message = api.last_error()
        assert rc == F.HK_E_INVALID, (what, rc, message)
        assert "item 6" in message, (what, message)
    assert scene_bytes(p, meshes) == before, "a refused batch wrote to the scene"
    # the set call's own refusals
    raw = api.raw("set_mesh_morph_targets")
    m = meshes[names[0]]
    fp = lambda a: a.ctypes.data_as(C.POINTER(F.f32))
    nv = len(m["rest"])
    args = [ctx, C.byref(m["index"]), nv, 5, fp(m["rest"]), fp(m["normals"]), fp(m["dp"]), fp(m["dn"])]
    for k, value in ((3, 0), (3, F.MORPH_MAX_TARGETS + 1), (2, nv - 1), (2, nv + 1), (2, 0), (4, None), (5, None), (6, None), (1, None)):
        bad = list(args)
        bad[k] = value
        assert raw(*bad) == F.HK_E_INVALID, (k, value)
    unknown = F.HkMeshIndex(m["index"].vertex, m["index"].primitive, m["index"].node_offset + 1, m["index"].node_count)
    assert raw(ctx, C.byref(unknown), *args[2:]) == F.HK_E_INVALID
    p.engine.deform_meshes(good)                 # the set the refused calls named is still the old one
    assert scene_bytes(p, meshes) == before


# ---- 8
def test_morph_composes_with_refits_rebuilds_and_added_meshes():
    (gpu, gs, gm), (twin, ts, tm), sun = make_pair("yard", MAIN)
    cam, lights, s = frame_tools(sun)
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)

    def step(n, what, act):
        act(gpu, gs)
        act(twin, ts)
        gpu.engine.deform_meshes(items_of(gm, n + 2))
        twin_calls(twin.engine, tm, items_of(tm, n + 2))
        for p in (gpu, twin):
            p.render(cam, s, lights=lights, frame_number=n)
        assert_same_frame(gpu, twin, what)
        assert_same_scene(gpu, twin, gm, tm, what)

    mover = len(gs.instances) - 2
    rest = np.ctypeslib.as_array(gs.instances[mover].model).copy()

    def refit(p, scene):
        moved = rest.copy()
        moved[12] += 0.2
        scene.builder.set_instance_transform(mover, moved)
        assert p.engine.refit_instances(scene.builder) == 1

    def rebuild(p, scene):
        meshes = gm if p is gpu else tm
        p.engine.rebuild_mesh_tree(meshes["m5"]["index"], F.TREE_SAH)   # 722 triangles, 300 targets: the refit climbs the new topology

    def add(p, scene):
        q, qn, uv, idx = S.coil_ribbon(333)
        scene.builder.add_mesh(q, qn, uv, idx, build_tree=False)   # (its tree is built on the device)
        scene.builder.finish()
        p.add_meshes(scene.builder)
        assert p.engine.last_add()[:2] == (1, 333) and p.engine.last_add()[4] == 1   # (the scene moved to a larger allocation)

    step(2, "a morph batch after an instance refit", refit)
    step(3, "a morph batch after a mesh tree rebuild", rebuild)
    step(4, "a morph batch after hk_add_meshes with a growth move", add)


# ---- 9
def test_a_set_given_again_takes_effect_and_an_upload_drops_it():
    (gpu, gs, gm), (twin, ts, tm), sun = make_pair("small", SMALL)
    cam, lights, s = frame_tools(sun)
    names = ["m0", "m1"]
    for meshes in (gm, tm):
        for name in names:
            m = meshes[name]
            m["dp"], m["dn"] = S.morph_targets(m["rest"], m["normals"], m["targets"], seed=99 + m["k"], normal_deltas=name == "m1")
            m["dp"] = (m["dp"] * np.float32(1.5)).astype(np.float32)
    for name in names:
        m = gm[name]
        gpu.engine.set_mesh_morph_targets(m["index"], m["rest"], m["normals"], m["dp"], m["dn"])
    gpu.engine.deform_meshes(items_of(gm, 2))
    twin_calls(twin.engine, tm, items_of(tm, 2))
    for p in (gpu, twin):
        p.render(cam, s, lights=lights, frame_number=1)
    assert_same_frame(gpu, twin, "other deltas")
    assert_same_scene(gpu, twin, gm, tm, "other deltas")
    # hk_upload_scene drops the sets, as it drops skins
    gpu.set_scene(gs)
    api, ctx = gpu.engine.api, gpu.engine.ctx
    for item in (items_of(gm, 3)[0], items_of(gm, 3)[1]):
        table, keep = deform_items([item])
        assert api.raw("deform_meshes")(ctx, table, 1) == F.HK_E_INVALID
        assert "item 0" in api.last_error() and "morph set" in api.last_error()
    assert api.raw("upload_scene_instances")(ctx, gs.builder.h) == F.HK_OK   # nothing was deformed since the upload
    set_up(gpu.engine, gm)
    gpu.engine.deform_meshes(items_of(gm, 3))


# ---- 10
def test_bands_take_morph_items_like_the_single_context():
    from bevy_hikari_amd.distributed import MultiEngine

    scene, sun, meshes = build_scene("small", SMALL)
    s = hk.HikariSettings(indirect_bounces=2, upscale=hk.Upscale.SMAA_TU_1_0)
    w, h = 96, 64
    cam, lights = S.synthetic_camera(w, h), hk.lights_uniform(directional=sun)
    view, pview = cam.view_uniform(), cam.previous_view_uniform()
    m, ref = MultiEngine([0, 0], flags=F.CTX_DETERMINISTIC_SCATTER), hk.Engine(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
    for t in (m, ref):
        t.upload_noise(); t.upload_scene(scene); t.resize(w, h, 1.0)
        set_up(t, meshes)
    m.set_band_bounds([0, 20, 64])
    for n in range(1, 4):
        if n > 1:
            m.deform_meshes(items_of(meshes, n))
            ref.deform_meshes(items_of(meshes, n))
        f = hk.frame_uniform(s, n)
        m.frame_render(f, view, pview, lights, s.to_c())
        ref.frame_render(f, view, pview, lights, s.to_c())
        m.wait(); ref.wait()
        for b in (F.BUF_TONE_MAPPED, F.BUF_POSITION, F.BUF_NORMAL, F.BUF_RENDER0 + 2, F.BUF_DENOISE_RENDER0 + 2):
            assert (m.read(b).view(np.uint8) == ref.read(b).view(np.uint8)).all(), f"frame {n}: buffer {b} differs"
    for name in ("m0", "m1"):
        want = hk.morph_vertices(meshes[name]["rest"], meshes[name]["normals"], meshes[name]["dp"], meshes[name]["dn"], weights_of(meshes[name], 3))
        geo = ref.read_mesh_geometry(meshes[name]["index"])
        if meshes[name]["kind"] == "morph":
            assert np.ascontiguousarray(geo["positions"][:, :3]).tobytes() == want[0].tobytes()
        for band_geo in m.read_mesh_geometry(meshes[name]["index"]):
            for key in ("positions", "normals", "triangles", "box"):
                assert band_geo[key].tobytes() == geo[key].tobytes(), f"{name}: {key} differ"
