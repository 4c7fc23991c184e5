"""Instance poses from device memory (hk_set_instance_transforms_device).  The yardstick is a TWIN context given the same poses through its
builder and hk_refit_scene_instances: after every frame every screen-space buffer, both instance-level trees and the emitter records with
their alias tables must be equal byte for byte.  Moving objects make the reference's scatter race observable: both contexts resolve it
(HK_CTX_DETERMINISTIC_SCATTER), and emissive spatial reuse is on so that no channel keeps the race.

Shapes: the Cornell box (8 instances under one transform, one slot, refit in place); a yard of 409 instances and 8 emitters beyond the LDS
copy (two slots, eight direction-threaded orderings; 409 = six full workgroups of the per-instance kernels and one of 25); a small yard
for the cases about sources, ordering and state."""
import ctypes as C
import math

import numpy as np
import pytest

import bevy_hikari_amd as hk
from bevy_hikari_amd import _ffi as F
from bevy_hikari_amd import scenes as S
from bevy_hikari_amd.scenes import synthetic_camera, synthetic_large, synthetic_scene
from cases import _as_float, diff_buffers, product_default_traversal, snapshot

pytestmark = pytest.mark.gpu

SMALL = dict(n_boxes=3, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)    # 6 instances; fits the LDS copy: one slot
SIZE = (96, 64)


def torch_():
    import torch

    return torch


def pose(rest, frame, k):
    """a finite, invertible pose near `rest` (16 floats, column-major) that differs from frame to frame"""
    m = rest.reshape(4, 4).T.astype(np.float64)
    ang = 0.07 * frame * (1 + k % 5)
    c, s = math.cos(ang), math.sin(ang)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=np.float64)
    shift = np.eye(4)
    shift[0, 3] = 0.05 * frame * (1 if k % 2 == 0 else -1)
    shift[1, 3] = 0.02 * frame * (k % 3 == 0)
    return (shift @ m @ rot).T.astype(np.float32).reshape(-1)


def large_yard():
    return synthetic_large(0x5EED0007, 4, 6, 8, 400, 20, 8, 12.0)   # ground + 400 rocks of 4 small meshes + 8 emissive quads


class Twin:
    """`dev` receives poses through torch tensors and the new call, `ref` through its builder and refit_instances"""

    def __init__(self, make, camera=None, default_traversal=False, settings=None):
        self.plugins, self.scenes = [], []
        for _ in range(2):
            scene, self.sun = make()
            if default_traversal:
                with product_default_traversal():
                    p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
            else:
                p = hk.HikariPlugin(device=0, flags=F.CTX_DETERMINISTIC_SCATTER)
            p.set_scene(scene)
            self.plugins.append(p)
            self.scenes.append(scene)
        self.dev, self.ref = self.plugins
        self.dev_scene, self.ref_scene = self.scenes
        self.n = len(self.dev_scene.instances)
        self.rest = np.array([np.ctypeslib.as_array(i.model).copy() for i in self.dev_scene.instances], dtype=np.float32)
        self.current = self.rest.copy()            # what both devices are meant to hold
        self.emitters = sorted(int(e.instance) for e in self.dev_scene.emissives)
        self.cam = camera or synthetic_camera(*SIZE)
        self.lights = hk.lights_uniform(directional=self.sun) if self.sun else hk.lights_uniform()
        self.settings = settings or hk.HikariSettings(indirect_bounces=2, emissive_spatial_reuse=True, upscale=hk.Upscale.SMAA_TU_1_0)
        self.device = torch_().device("cuda", 0)

    def tensor(self, array):
        return torch_().from_numpy(np.ascontiguousarray(array, dtype=np.float32)).to(self.device)

    def move_ref(self, poses):
        """poses {instance: 16 floats} on the twin's builder, then hk_refit_scene_instances; returns how many it found moved"""
        for i, m in poses.items():
            self.ref_scene.builder.set_instance_transform(int(i), m)
        return self.ref.engine.refit_instances(self.ref_scene.builder)

    def move(self, poses, named=True, **kw):
        """Both contexts to `poses` {instance: 16 floats}.  named: the device call names exactly these instances, in the dict's order;
        otherwise it passes the poses of all instances with ids=None."""
        moved = {i: m for i, m in poses.items() if m.tobytes() != self.current[i].tobytes()}
        for i, m in poses.items():
            self.current[i] = m
        if named:
            ids = [int(i) for i in poses]
            self.dev.engine.set_instance_transforms(self.dev_scene.builder, self.tensor(self.current[ids]), ids=ids, **kw)
        else:
            self.dev.engine.set_instance_transforms(self.dev_scene.builder, self.tensor(self.current), **kw)
        assert self.move_ref(poses) == len(moved)

    def render(self, n):
        for p in self.plugins:
            p.render(self.cam, self.settings, lights=self.lights, frame_number=n)

    def assert_same(self, what):
        a, b = self.dev.engine, self.ref.engine
        counts = len(self.dev_scene.instance_nodes), len(self.dev_scene.emissive_nodes)
        for x, y, name in zip(a.read_trees(*counts), b.read_trees(*counts), ("instance tree", "light tree")):
            assert bytes(x) == bytes(y), f"{what}: the {name} differs"
        (ra, aa), (rb, ab) = a.read_emitters(), b.read_emitters()
        assert ra.tobytes() == rb.tobytes() and aa.tobytes() == ab.tobytes(), f"{what}: emitter records / alias tables differ"
        bad = diff_buffers(snapshot(self.dev), snapshot(self.ref))
        assert bad == {}, f"{what}: {bad}"

    def velocity_of(self, plugin, instance):
        """|velocity_uv| over the pixels whose primary ray hit `instance` (the plane holds instance + 0.5)"""
        seen = plugin.engine.read(F.BUF_INSTANCE_MATERIAL)[..., 0] == instance + 0.5
        assert seen.mean() > 0.02, "the instance must be in view"
        return np.abs(_as_float(plugin.engine.read(F.BUF_VELOCITY_UV))[..., :2][seen])


# ---- 1
def test_cornell_three_of_eight_move_one_of_them_the_emitter():
    twin = Twin(lambda: (hk.load_cornell(), None), camera=hk.cornell_camera(*SIZE))
    assert twin.n == 8 and len({m.tobytes() for m in twin.rest}) == 1, "the premise: eight instances under one transform"
    emitter = twin.emitters[0]
    movers = [1, emitter, [i for i in range(8) if i not in (1, emitter)][-1]]
    twin.render(1)
    twin.assert_same("frame 1")
    for n in range(2, 6):
        twin.move({i: pose(twin.rest[i], n - 1, k) for k, i in enumerate(movers)})
        assert twin.dev.engine.traversal_mode()[0] != "one-level"     # the host no longer knows whether the transforms are shared
        twin.render(n)
        twin.assert_same(f"frame {n}")
    st = twin.dev.engine.stats()
    assert st.scene_device_refits == 4


# ---- 2, 11
def test_two_slot_scene_a_random_seventh_moves_per_frame_by_id():
    twin = Twin(large_yard, camera=synthetic_camera(*SIZE, extent=12.0), default_traversal=True)
    rng = np.random.default_rng(7)
    twin.render(1)
    assert twin.n == 409 and len(twin.emitters) == 8 and twin.dev.engine.traversal_mode() == ("threaded", 8)
    before = twin.dev.engine.stats()
    for n in range(2, 6):
        chosen = rng.choice(twin.n, size=61, replace=False)          # 15 %, in no particular order
        ids = [int(i) for i in chosen] + [e for e in twin.emitters[:n] if e not in chosen]   # ... with emitters among them, not in front
        twin.move({i: pose(twin.rest[i], n - 1, k) for k, i in enumerate(ids)})
        twin.render(n)
        twin.assert_same(f"frame {n}")
    st = twin.dev.engine.stats()
    assert st.scene_device_refits == before.scene_device_refits + 4                      # one per call
    assert st.scene_instance_builds == before.scene_instance_builds and st.scene_async_instance_uploads == before.scene_async_instance_uploads


# ---- 3
def test_all_poses_given_and_only_some_changed():
    twin = Twin(large_yard, camera=synthetic_camera(*SIZE, extent=12.0), default_traversal=True)
    ground = 0                                                        # the slab under everything: in view in every frame
    twin.render(1)
    a, b = [ground, 5, 77, 300, twin.emitters[2]], [9, 120, 408, twin.emitters[0]]
    twin.move({i: pose(twin.rest[i], 2, k) for k, i in enumerate(a)}, named=False)
    twin.render(2)
    twin.assert_same("frame 2: a moves")
    moving = twin.velocity_of(twin.dev, ground).max()
    twin.move({i: pose(twin.rest[i], 3, k) for k, i in enumerate(b)}, named=False)       # a rests where it is, b moves
    twin.render(3)
    twin.assert_same("frame 3: a rests, b moves")
    resting = twin.velocity_of(twin.dev, ground).max()
    assert moving > 4 * resting, (moving, resting)                   # `moved` was cleared and previous model = model
    twin.move({}, named=False)                                        # every pose as the device holds it
    twin.render(4)
    twin.assert_same("frame 4: everything rests")
    twin.move({i: pose(twin.rest[i], 5, k) for k, i in enumerate(a)}, named=False)
    twin.render(5)
    twin.assert_same("frame 5: a moves again")


# ---- 4
def test_an_instance_moved_by_one_call_and_not_named_by_the_next_is_at_rest():
    twin = Twin(large_yard, camera=synthetic_camera(*SIZE, extent=12.0), default_traversal=True)
    ground = 0
    twin.render(1)
    twin.move({i: pose(twin.rest[i], 2, k) for k, i in enumerate([ground, 40, twin.emitters[1]])})
    twin.render(2)
    twin.assert_same("frame 2")
    moving = twin.velocity_of(twin.dev, ground).max()
    twin.move({i: pose(twin.rest[i], 3, k) for k, i in enumerate([41, 42])})             # neither the ground nor the emitter is named
    twin.render(3)
    twin.assert_same("frame 3")
    resting = twin.velocity_of(twin.dev, ground)
    assert moving > 4 * resting.max(), (moving, resting.max())
    assert resting.tobytes() == twin.velocity_of(twin.ref, ground).tobytes()
    twin.move({ground: twin.current[ground].copy(), 43: pose(twin.rest[43], 4, 0)})       # ... and named with the pose it has: at rest as well
    twin.render(4)
    twin.assert_same("frame 4")
    assert twin.velocity_of(twin.dev, ground).tobytes() == twin.velocity_of(twin.ref, ground).tobytes()


# ---- 5
def test_strided_sources_and_an_odd_offset():
    torch = torch_()
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    ids = [1, 4, twin.n - 1]
    for n, offset in ((2, 0), (3, 1), (4, 3)):
        poses = {i: pose(twin.rest[i], n - 1, k) for k, i in enumerate(ids)}
        storage = torch.full((len(ids) * 24 + 8,), 7.5, dtype=torch.float32, device=twin.device)
        wide = storage[offset:offset + len(ids) * 24].view(len(ids), 24)   # offset 0: 16-byte aligned rows of 96 bytes; 1, 3: 4-byte aligned only
        wide[:, :16] = twin.tensor(np.stack([poses[i] for i in ids]))
        source = wide[:, :16]
        assert source.stride(0) == 24 and source.data_ptr() % 16 == (4 * offset) % 16
        for i in ids:
            twin.current[i] = poses[i]
        twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, source, ids=ids)
        assert twin.move_ref(poses) == len(ids)
        twin.render(n)
        twin.assert_same(f"frame {n}, source {offset} floats into its storage")
    pose44 = {i: pose(twin.rest[i], 6, k) for k, i in enumerate(ids)}                      # ... and the (n, 4, 4) form
    for i in ids:
        twin.current[i] = pose44[i]
    twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, twin.tensor(np.stack([pose44[i] for i in ids])).view(-1, 4, 4), ids=ids)
    assert twin.move_ref(pose44) == len(ids)
    twin.render(5)
    twin.assert_same("frame 5, poses of shape (n, 4, 4)")


# ---- 6
def test_the_producer_stream_is_ordered_before_and_after_the_call():
    torch = torch_()
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    ids = [2, twin.n - 1]
    first = np.stack([pose(twin.rest[i], 3, k) for k, i in enumerate(ids)])
    half = twin.tensor(first * np.float32(0.5))         # (x 2 on the device is exact: the twin is given `first` itself)
    busy = torch.randn((2048, 2048), device=twin.device)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(twin.device)
    with torch.cuda.stream(stream):
        for _ in range(8):                               # the producing kernel is queued behind work that takes a while
            busy = torch.mm(busy, busy) * 1e-3
        models = half * 2.0
        twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, models, ids=ids, producer_stream=stream)
        models.zero_()                                   # overwritten in stream order right after the call
    assert twin.move_ref({i: first[k] for k, i in enumerate(ids)}) == 2
    twin.render(2)
    twin.assert_same("poses produced on a side stream, then overwritten")
    stream.synchronize()
    assert twin.dev.engine.read_instance_transforms()[ids].tobytes() == first.tobytes()


# ---- 7
def test_a_moved_instance_of_a_deformed_mesh_keeps_the_devices_mesh_box():
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    box_positions = np.ascontiguousarray(S._box()[0], dtype=np.float32).reshape(-1, 3)
    grown = (box_positions * np.float32(1.4)).astype(np.float32)
    for p, scene in zip(twin.plugins, twin.scenes):
        p.engine.deform_meshes([("vertices", scene.builder.mesh_index(0), grown, None)])   # mesh 0: the box of instances 0 .. 3
    twin.render(2)
    twin.assert_same("frame 2: the box mesh deformed")
    twin.move({i: pose(twin.rest[i], 2, k) for k, i in enumerate([1, 2, twin.n - 1])})    # the builders still hold the old box
    twin.render(3)
    twin.assert_same("frame 3: instances of the deformed mesh moved")
    twin.move({i: pose(twin.rest[i], 3, k) for k, i in enumerate([1])}, named=False)
    twin.render(4)
    twin.assert_same("frame 4")


# ---- 8
def test_a_singular_and_a_non_finite_pose_are_skipped_and_reported():
    torch = torch_()
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    good = {1: pose(twin.rest[1], 2, 0), twin.n - 1: pose(twin.rest[twin.n - 1], 2, 1)}
    singular, nan = pose(twin.rest[2], 2, 2), pose(twin.rest[4], 2, 3)
    singular[4:8] = 0.0                                  # a zero column
    nan[13] = np.nan
    ids = [1, 4, twin.n - 1, 2]
    rows = np.stack([good[1], nan, good[twin.n - 1], singular])
    status = torch.full((1,), 77, dtype=torch.int32, device=twin.device)
    for i, m in good.items():
        twin.current[i] = m
    twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, twin.tensor(rows), ids=ids, status=status)
    assert twin.move_ref(good) == 2                      # the twin never hears of the two others
    twin.render(2)
    twin.dev.engine.wait()
    assert int(status.item()) == 1 + 4                   # the highest offending instance id
    twin.assert_same("frame 2: instances 2 and 4 keep their poses")
    got = twin.dev.engine.read_instance_transforms()
    assert got.tobytes() == twin.current.tobytes()
    rows[3, 4:8] = np.inf                                # ... and an infinity alone, lower id: the word is written anew by every call
    rows[1] = pose(twin.rest[4], 3, 3)
    twin.current[4] = rows[1]
    twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, twin.tensor(rows), ids=ids, status=status)
    assert twin.move_ref({4: rows[1]}) == 1
    twin.render(3)
    twin.dev.engine.wait()
    assert int(status.item()) == 1 + 2
    twin.assert_same("frame 3")
    twin.dev.engine.set_instance_transforms(twin.dev_scene.builder, twin.tensor(rows[:3]), ids=ids[:3], status=status)
    twin.dev.engine.wait()
    assert int(status.item()) == 0


# ---- 9
def test_state_after_the_call_and_the_way_back():
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    movers = [1, 4, twin.n - 1]
    twin.move({i: pose(twin.rest[i], 2, k) for k, i in enumerate(movers)})
    twin.render(2)
    twin.assert_same("frame 2")
    e, b = twin.dev.engine, twin.dev_scene.builder
    for call in (lambda: e.refit_instances(b), lambda: e.update_instances_on_device(b)):
        with pytest.raises(hk.HikariError) as err:
            call()
        assert err.value.code == F.HK_E_NOT_READY and "hk_read_instance_transforms" in str(err.value)
    # what works from device state stays usable, and leaves both contexts equal
    for p, scene in zip(twin.plugins, twin.scenes):
        m = F.HkMaterial.from_buffer_copy(bytes(scene.materials[2]))
        m.base_color[0], m.base_color[1] = 0.9, 0.1
        scene.builder.set_material(2, m)
        assert p.engine.update_materials(scene.builder) == 1
        p.engine.rebuild_trees(F.TREE_SAH)
    rays = np.zeros((4, 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 3], rays[:, 5] = np.linspace(-1.5, 1.5, 4), 6.0, 0.2, 100.0, -1.0   # straight down onto the yard
    rays.view(np.uint32)[:, 7] = F.NO_INSTANCE
    hits = [p.engine.cast_rays(rays.copy()) for p in twin.plugins]
    assert (hits[0]["status"] == F.RAY_HIT).all() and hits[0].tobytes() == hits[1].tobytes()
    twin.render(3)
    twin.assert_same("frame 3: material edit, tree rebuild and ray queries after the call")
    # the way back
    got = e.read_instance_transforms()
    assert got.shape == (twin.n, 16) and got.tobytes() == twin.current.tobytes()
    with pytest.raises(hk.HikariError):
        e.refit_instances(b)                             # reading alone does not end the state
    for i in range(twin.n):
        b.set_instance_transform(i, got[i])
    b.finish()                                           # (the builder was not told when they moved: a second finish makes these its previous
    e.upload_instances(b.finish())                       #  poses too, as the twin's builder has held them since frame 2)
    twin.ref.engine.upload_instances(twin.ref_scene.builder.finish())
    twin.render(4)
    twin.assert_same("frame 4: both uploaded from their builders")
    step = {i: pose(twin.rest[i], 4, k) for k, i in enumerate(movers)}
    for i, m in step.items():
        b.set_instance_transform(i, m)
        twin.current[i] = m
    assert e.refit_instances(b) == len(movers)           # the host path works again
    assert twin.move_ref(step) == len(movers)
    twin.render(5)
    twin.assert_same("frame 5: refit through the builder again")


# ---- 10
def test_refused_calls_write_nothing():
    torch = torch_()
    twin = Twin(lambda: synthetic_scene(**SMALL))
    twin.render(1)
    e, b, api = twin.dev.engine, twin.dev_scene.builder, twin.dev.engine.api
    call = api.raw("set_instance_transforms_device")
    models = twin.tensor(np.stack([pose(twin.rest[i], 2, k) for k, i in enumerate(range(twin.n))]))
    ptr = models.data_ptr()
    host = np.ascontiguousarray(twin.rest)
    status = torch.zeros((1,), dtype=torch.int32, device=twin.device)
    other, _ = synthetic_scene(n_boxes=5, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)

    def ids(*values):
        return (F.u32 * len(values))(*values)

    before = bytes(e.stats())
    cases = {
        "NULL ctx": (None, b.h, ids(1, 2), 2, ptr, 64, None, None),
        "NULL builder": (e.ctx, None, ids(1, 2), 2, ptr, 64, None, None),
        "NULL poses": (e.ctx, b.h, ids(1, 2), 2, None, 64, None, None),
        "ids for no instance": (e.ctx, b.h, ids(1), 0, ptr, 64, None, None),
        "an id beyond the scene": (e.ctx, b.h, ids(1, twin.n), 2, ptr, 64, None, None),
        "more poses than instances": (e.ctx, b.h, None, twin.n + 1, ptr, 64, None, None),
        "an id named twice": (e.ctx, b.h, ids(1, 3, 1), 3, ptr, 64, None, None),
        "a stride of 60": (e.ctx, b.h, ids(1, 2), 2, ptr, 60, None, None),
        "a stride of 66": (e.ctx, b.h, ids(1, 2), 2, ptr, 66, None, None),
        "a misaligned pointer": (e.ctx, b.h, ids(1, 2), 2, ptr + 2, 64, None, None),
        "a pageable host pointer": (e.ctx, b.h, ids(1, 2), 2, host.ctypes.data, 64, None, None),
        "an extent beyond the allocation": (e.ctx, b.h, ids(1, 2, 3), 3, ptr, 1 << 30, None, None),
        "a misaligned status word": (e.ctx, b.h, ids(1, 2), 2, ptr, 64, None, status.data_ptr() + 1),
        "a host status word": (e.ctx, b.h, ids(1, 2), 2, ptr, 64, None, host.ctypes.data),
        "another scene's builder": (e.ctx, other.builder.h, ids(1, 2), 2, ptr, 64, None, None),
    }
    for what, args in cases.items():
        rc = call(*args)
        assert rc == F.HK_E_INVALID, (what, rc, api.last_error())
        if args[0] is not None:
            assert bytes(e.stats()) == before, what
    assert e.last_pose() == (0, 0)                       # nothing was ever enqueued
    empty = hk.Engine(device=0)
    assert call(empty.ctx, b.h, ids(1), 1, ptr, 64, None, None) == F.HK_E_NOT_READY
    assert api.raw("read_instance_transforms")(empty.ctx, host.ctypes.data_as(C.POINTER(F.f32)), twin.n) == F.HK_E_NOT_READY
    assert api.raw("read_instance_transforms")(e.ctx, host.ctypes.data_as(C.POINTER(F.f32)), twin.n + 1) == F.HK_E_INVALID
    torch.cuda.synchronize()
    twin.render(2)
    twin.assert_same("after the refusals")                # the twin made no call at all
    assert e.refit_instances(b) == 0                      # nothing is stale either


# ---- 12
def test_launch_count_does_not_depend_on_how_many_instances_are_named():
    twin = Twin(large_yard, camera=synthetic_camera(*SIZE, extent=12.0), default_traversal=True)
    twin.render(1)
    few = [3, twin.emitters[0]]
    twin.move({i: pose(twin.rest[i], 2, k) for k, i in enumerate(few)})
    assert twin.dev.engine.last_pose() == (6, 1)          # begin, records, instances, emitters, two trees; the first call copies the mesh boxes
    many = list(range(1, 300)) + twin.emitters
    twin.move({i: pose(twin.rest[i], 3, k) for k, i in enumerate(many)})
    assert twin.dev.engine.last_pose() == (6, 0)          # ... a warm call copies nothing per instance
    twin.move({i: pose(twin.rest[i], 4, k) for k, i in enumerate(many)}, named=False)
    assert twin.dev.engine.last_pose() == (6, 0)
    twin.move({5: pose(twin.rest[5], 5, 0)})              # no emitter named: its launch is not made
    assert twin.dev.engine.last_pose() == (5, 0)
    twin.render(2)
    twin.assert_same("after four calls")
