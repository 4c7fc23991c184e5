"""Seeded synthetic scenes standing in for the reference's missing assets (scene.gltf,
City/scene.bin and the Low Poly glbs are absent from the checkout).  Pure data generation; all
acceleration structures are built by the library (SceneBuilder)."""
import math

import numpy as np

from . import _ffi as F
from .plugin import SceneBuilder, standard_material


def _box(sx=1.0, sy=1.0, sz=1.0):
    """24-vertex box centred at the origin with per-face normals/uvs, 12 triangles (triangle list)."""
    p, n, uv, idx = [], [], [], []
    faces = [((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1), (0, 1, 0)), ((0, 1, 0), (0, 0, 1), (1, 0, 0)),
             ((0, -1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0), (1, 0, 0))]
    half = np.array([sx, sy, sz]) * 0.5
    for nrm, u, v in faces:
        nrm, u, v = np.array(nrm, float), np.array(u, float), np.array(v, float)
        base = len(p)
        for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            p.append((nrm + a * u + b * v) * half)
            n.append(nrm)
            uv.append(((a + 1) / 2, (b + 1) / 2))
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(p, np.float32), np.array(n, np.float32), np.array(uv, np.float32), np.array(idx, np.uint32)


def _quad_strip(nx=4):
    """A unit XZ quad (normal +Y) tessellated as ONE triangle strip of 2*nx triangles (exercises the
    strip winding rule, mod.rs:432-449)."""
    p, n, uv = [], [], []
    for i in range(nx + 1):
        x = i / nx - 0.5
        for z in (0.5, -0.5):
            p.append((x, 0.0, z))
            n.append((0.0, 1.0, 0.0))
            uv.append((i / nx, z + 0.5))
    return np.array(p, np.float32), np.array(n, np.float32), np.array(uv, np.float32)


def _sphere(rings=8, segs=12):
    p, n, uv, idx = [], [], [], []
    for r in range(rings + 1):
        th = math.pi * r / rings
        for s in range(segs + 1):
            ph = 2 * math.pi * s / segs
            d = (math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph))
            p.append(tuple(0.5 * c for c in d))
            n.append(d)
            uv.append((s / segs, r / rings))
    for r in range(rings):
        for s in range(segs):
            a = r * (segs + 1) + s
            b = a + segs + 1
            idx += [a, a + 1, b, a + 1, b + 1, b]
    return np.array(p, np.float32), np.array(n, np.float32), np.array(uv, np.float32), np.array(idx, np.uint32)


def _trs(t, angles, s):
    ax, ay, az = angles
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = (ry @ rx @ rz) * np.asarray(s, float)[None, :]
    m[:3, 3] = t
    return m.T.astype(np.float32).reshape(-1)  # column-major


def _test_textures(rng):
    """Four small procedural RGBA8 images covering the sampler variants (sRGB / linear format,
    bilinear / nearest, repeat / mirror / clamp)."""
    yy, xx = np.mgrid[0:16, 0:32]
    checker = np.where(((xx // 4 + yy // 4) % 2)[..., None] == 0, np.array([230, 60, 40, 255]), np.array([40, 90, 220, 255])).astype(np.uint8)
    stripes = np.zeros((8, 8, 4), np.uint8)
    stripes[..., 3] = 255
    stripes[:, ::2, :3] = (200, 200, 190)
    stripes[:, 1::2, :3] = (90, 120, 60)
    noise = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    glow = np.zeros((4, 16, 4), np.uint8)
    glow[..., 3] = 255
    glow[..., 0] = np.linspace(40, 255, 16).astype(np.uint8)[None, :]
    glow[..., 1] = 180
    glow[..., 2] = np.linspace(255, 30, 16).astype(np.uint8)[None, :]
    return [dict(rgba=checker, srgb=True, linear=True, address_u=F.ADDRESS_REPEAT, address_v=F.ADDRESS_REPEAT),
            dict(rgba=stripes, srgb=True, linear=False, address_u=F.ADDRESS_MIRROR_REPEAT, address_v=F.ADDRESS_CLAMP_TO_EDGE),
            dict(rgba=noise, srgb=False, linear=True, address_u=F.ADDRESS_CLAMP_TO_EDGE, address_v=F.ADDRESS_MIRROR_REPEAT),
            dict(rgba=glow, srgb=True, linear=True, address_u=F.ADDRESS_REPEAT, address_v=F.ADDRESS_CLAMP_TO_EDGE)]


def synthetic_scene(seed=0x5EED0003, n_boxes=24, n_spheres=6, n_emitters=4, extent=4.0, sphere_rings=8, sphere_segs=12, textured=False, n_emissive_spheres=0):
    """A room-less yard: ground slab, random boxes and spheres with rotated / non-uniformly scaled
    instances of a few shared meshes, `n_emitters` emissive strip-quads above it.  Returns
    (SceneData, suggested sun dict).  textured=True binds four procedural textures (base colour,
    metallic, occlusion, emissive; light.wgsl:749-793)."""
    rng = np.random.default_rng(seed)
    b = SceneBuilder()
    box = b.add_mesh(*_box())
    sp = _sphere(sphere_rings, sphere_segs)
    sphere = b.add_mesh(*sp)
    qp, qn, quv = _quad_strip(4)
    quad = b.add_mesh(qp, qn, quv, None, F.TOPOLOGY_TRIANGLE_STRIP)
    mats = [b.add_material(standard_material(tuple(rng.uniform(0.2, 0.9, 3)) + (1.0,), (0, 0, 0), float(rng.uniform(0.3, 1.0)),
                                             float(rng.choice([0.0, 0.0, 1.0])), 0.5)) for _ in range(8)]
    emat = [b.add_material(standard_material((0.8, 0.8, 0.8, 1.0), tuple(rng.uniform(0.2, 1.0, 3)), 1.0, 0.0, 0.5)) for _ in range(max(1, n_emitters))]
    textures = []
    if textured:
        textures = _test_textures(rng)

        def mat(base=(1, 1, 1, 1), emissive=(0, 0, 0), rough=0.6, metallic=0.0, **ids):
            m = standard_material(base, emissive, rough, metallic, 0.5)
            for k, v in ids.items():
                setattr(m, k, v)
            return b.add_material(m)

        mats[0] = mat((0.9, 0.9, 0.9, 1), base_color_texture=1)                                   # ground: nearest / mirror / clamp
        mats[1] = mat((1, 1, 1, 1), base_color_texture=0)                                         # checker, bilinear repeat
        mats[2] = mat((0.8, 0.7, 0.6, 1), rough=0.4, metallic=1.0, metallic_roughness_texture=2)  # metallic *= noise.r
        mats[3] = mat((0.7, 0.8, 0.9, 1), base_color_texture=0, occlusion_texture=2)
        emat[0] = mat((0.8, 0.8, 0.8, 1), (1.0, 0.9, 0.8), 1.0, emissive_texture=3)
    # ground
    b.add_instance(box, mats[0], _trs((0, -0.25, 0), (0, 0, 0), (2.5 * extent, 0.5, 2.5 * extent)))
    for _ in range(n_boxes):
        t = (rng.uniform(-extent, extent), rng.uniform(0.2, 1.5), rng.uniform(-extent, extent))
        b.add_instance(box, mats[int(rng.integers(1, 8))], _trs(t, rng.uniform(-0.6, 0.6, 3), rng.uniform(0.3, 1.4, 3)))
    for _ in range(n_spheres):
        t = (rng.uniform(-extent, extent), rng.uniform(0.4, 1.8), rng.uniform(-extent, extent))
        b.add_instance(sphere, mats[int(rng.integers(1, 8))], _trs(t, rng.uniform(-1, 1, 3), rng.uniform(0.5, 1.5, 3)))
    for i in range(n_emitters):
        t = (rng.uniform(-extent, extent) * 0.8, rng.uniform(2.2, 3.2), rng.uniform(-extent, extent) * 0.8)
        # flipped so the strip's +Y normal faces down
        b.add_instance(quad, emat[i], _trs(t, (math.pi + rng.uniform(-0.3, 0.3), rng.uniform(-1, 1), 0.0), (rng.uniform(0.4, 1.0), 1.0, rng.uniform(0.4, 1.0))))
    for i in range(n_emissive_spheres):  # examples/scene.rs:231-235: an emissive sphere - an emitter with as many triangles as the sphere mesh
        t = (rng.uniform(-extent, extent) * 0.6, rng.uniform(1.6, 2.4), rng.uniform(-extent, extent) * 0.6)
        b.add_instance(sphere, emat[i % len(emat)], _trs(t, rng.uniform(-1, 1, 3), rng.uniform(0.25, 0.5, 3)))
    sun = dict(color=(1.0, 0.96, 0.9), illuminance=20000.0, direction_to_light=(0.35, 0.8, 0.45))
    scene = b.finish()
    scene.textures = textures
    scene.builder = b  # kept for dynamic-scene use: builder.set_instance_transform(i, ..) + builder.finish()
    return scene, sun


def animate(scene, frame, movers=(3, 9, 26, 31)):
    """Move a few instances of a synthetic_scene (two boxes, a sphere, an emitter) to their pose at
    `frame` and re-finish the builder.  Returns the new SceneData (meshes and materials unchanged;
    previous_transforms = the poses of the previous call).  Frame 0 is the rest pose."""
    b = scene.builder
    if not hasattr(scene, "rest_pose"):
        scene.rest_pose = np.array([np.ctypeslib.as_array(inst.model).copy() for inst in scene.instances], dtype=np.float32)
    for k, i in enumerate(movers):
        if i >= len(scene.rest_pose):
            continue
        m = scene.rest_pose[i].reshape(4, 4).T.astype(np.float64)  # column-major -> math layout
        ang = 0.05 * frame * (1 + k)
        c, s_ = math.cos(ang), math.sin(ang)
        rot = np.array([[c, 0, s_, 0], [0, 1, 0, 0], [-s_, 0, c, 0], [0, 0, 0, 1]], dtype=np.float64)
        shift = np.eye(4)
        shift[0, 3] = 0.04 * frame * (1 if k % 2 == 0 else -1)
        shift[1, 3] = 0.02 * frame * (k % 3 == 0)
        t = shift @ m @ rot  # spin about the local Y axis, drift in world space
        b.set_instance_transform(i, t.T.astype(np.float32).reshape(-1))
    new = b.finish()
    new.textures = getattr(scene, "textures", [])
    new.builder, new.rest_pose = b, scene.rest_pose
    return new


def synthetic_camera(width, height, extent=4.0):
    from .plugin import Camera, look_at_transform

    return Camera(look_at_transform((1.6 * extent, 1.1 * extent, 2.0 * extent), (0.0, 0.6, 0.0)), width, height)


def _rock(rng, rings, segs):
    """A sphere displaced by a few random low-frequency lobes: a unique closed mesh per seed."""
    p, n, uv, idx = _sphere(rings, segs)
    d = p / np.linalg.norm(p, axis=1, keepdims=True)
    disp = np.ones(len(p))
    for _ in range(6):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        disp += rng.uniform(0.05, 0.25) * np.sin(rng.uniform(1.5, 5.0) * (d @ axis) + rng.uniform(0, 6.28))
    p = (d * (0.5 * disp)[:, None]).astype(np.float32)
    # smooth normals from the displaced surface (area-weighted face normals)
    nrm = np.zeros_like(p, dtype=np.float64)
    tri = idx.reshape(-1, 3)
    fn = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    for k in range(3):
        np.add.at(nrm, tri[:, k], fn)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 1e-12, nrm / np.maximum(ln, 1e-12), d)
    return p, nrm.astype(np.float32), uv, idx


def synthetic_large(seed=0x5EED0003, n_meshes=40, rings=40, segs=80, n_instances=400, n_materials=50, n_emitters=8, extent=12.0):
    """Sponza-class stand-in (~260 k unique triangles, ~400 instances, 50
    materials, 8 emissive quads, sun 100 000 lux).  `rings x segs x 2` triangles per unique mesh.
    City-class (config 4): synthetic_large(0x5EED0004, 60, 80, 160, 2000, 50, 1, 40.0)."""
    rng = np.random.default_rng(seed)
    b = SceneBuilder()
    box = b.add_mesh(*_box())
    rocks = [b.add_mesh(*_rock(rng, rings, segs)) for _ in range(n_meshes)]
    qp, qn, quv = _quad_strip(4)
    quad = b.add_mesh(qp, qn, quv, None, F.TOPOLOGY_TRIANGLE_STRIP)
    mats = [b.add_material(standard_material(tuple(rng.uniform(0.15, 0.9, 3)) + (1.0,), (0, 0, 0), float(rng.uniform(0.25, 1.0)),
                                             float(rng.choice([0.0, 0.0, 0.0, 1.0])), 0.5)) for _ in range(n_materials)]
    emat = [b.add_material(standard_material((0.8, 0.8, 0.8, 1.0), tuple(rng.uniform(0.3, 1.0, 3)), 1.0, 0.0, 0.5)) for _ in range(max(1, n_emitters))]
    b.add_instance(box, mats[0], _trs((0, -0.25, 0), (0, 0, 0), (2.5 * extent, 0.5, 2.5 * extent)))
    for i in range(n_instances):
        t = (rng.uniform(-extent, extent), rng.uniform(0.3, 2.5), rng.uniform(-extent, extent))
        s = rng.uniform(0.6, 2.2, 3)
        b.add_instance(rocks[int(rng.integers(0, n_meshes))], mats[int(rng.integers(1, n_materials))], _trs(t, rng.uniform(-3.1, 3.1, 3), s))
    for i in range(n_emitters):
        t = (rng.uniform(-extent, extent) * 0.8, rng.uniform(3.5, 5.0), rng.uniform(-extent, extent) * 0.8)
        b.add_instance(quad, emat[i], _trs(t, (math.pi + rng.uniform(-0.3, 0.3), rng.uniform(-1, 1), 0.0), (rng.uniform(0.8, 2.0), 1.0, rng.uniform(0.8, 2.0))))
    sun = dict(color=(1.0, 0.96, 0.9), illuminance=100000.0, direction_to_light=(0.35, 0.8, 0.45))
    scene = b.finish()
    scene.builder = b
    return scene, sun


def flight_helmet_scene():
    """The reference's textured glTF asset (assets/models/FlightHelmet, flattened by
    tools/make_fixtures.py: 6 meshes, 94 722 triangles, base-colour + occlusion/roughness/metal
    textures at 256^2) on a ground slab under one emissive quad and a sun.  Materials are what
    bevy_gltf 0.9.1 builds: factors, texture ids, reflectance 0.5; glTF samplers are linear + repeat.
    Returns (SceneData with .textures, sun dict, Camera factory)."""
    import os

    from .plugin import ASSETS, Camera, look_at_transform

    d = np.load(os.path.join(ASSETS, "flight_helmet.npz"))
    b = SceneBuilder()
    textures = [dict(rgba=d["textures"][i], srgb=bool(d["texture_srgb"][i]), address_u=F.ADDRESS_REPEAT, address_v=F.ADDRESS_REPEAT, linear=True)
                for i in range(len(d["textures"]))]
    mats = []
    for row in d["materials"]:
        m = standard_material(tuple(row[:4]), (0, 0, 0), float(row[4]), float(row[5]), 0.5)
        m.base_color_texture, m.metallic_roughness_texture, m.occlusion_texture = int(row[6]), int(row[7]), int(row[8])
        mats.append(b.add_material(m))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in d["instances"]:
        k = int(inst[0])
        mesh = b.add_mesh(d[f"mesh{k}_positions"], d[f"mesh{k}_normals"], d[f"mesh{k}_uvs"], d[f"mesh{k}_indices"])
        b.add_instance(mesh, mats[int(d[f"mesh{k}_material"][0])], inst[1:17])
        t = inst[1:17].reshape(4, 4).T
        p = d[f"mesh{k}_positions"] @ t[:3, :3].T + t[:3, 3]
        lo, hi = np.minimum(lo, p.min(axis=0)), np.maximum(hi, p.max(axis=0))
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    ground = b.add_material(standard_material((0.55, 0.55, 0.6, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    lamp = b.add_material(standard_material((0.8, 0.8, 0.8, 1.0), (1.0, 0.95, 0.85), 1.0, 0.0, 0.5))
    box = b.add_mesh(*_box())
    qp, qn, quv = _quad_strip(2)
    quad = b.add_mesh(qp, qn, quv, None, F.TOPOLOGY_TRIANGLE_STRIP)
    b.add_instance(box, ground, _trs((centre[0], lo[1] - 0.05 * extent, centre[2]), (0, 0, 0), (4 * extent, 0.1 * extent, 4 * extent)))
    b.add_instance(quad, lamp, _trs((centre[0] + 0.4 * extent, hi[1] + 0.6 * extent, centre[2] + 0.5 * extent), (math.pi, 0.3, 0.0),
                                    (0.6 * extent, 1.0, 0.6 * extent)))
    scene = b.finish()
    scene.textures = textures
    scene.builder = b
    sun = dict(color=(1.0, 0.96, 0.9), illuminance=15000.0, direction_to_light=(0.4, 0.8, 0.5))

    def camera(width, height):
        eye = (centre[0] + 0.9 * extent, centre[1] + 0.35 * extent, centre[2] + 1.5 * extent)
        return Camera(look_at_transform(eye, tuple(centre)), width, height)

    return scene, sun, camera


# ---------------------------------------------------------------------------------------------
# deforming meshes (hk_update_mesh_vertices / hk_skin_mesh): geometry and its motion, pure numpy
# ---------------------------------------------------------------------------------------------
def cloth_grid(nx=12, nz=12, size=1.0):
    """A flat (nx x nz)-quad grid in the xz plane around the origin, +Y normals: positions, normals, uvs, indices."""
    xs, zs = np.meshgrid(np.linspace(-0.5, 0.5, nx + 1), np.linspace(-0.5, 0.5, nz + 1), indexing="xy")
    p = np.stack([xs * size, np.zeros_like(xs), zs * size], -1).reshape(-1, 3).astype(np.float32)
    n = np.tile(np.array([0, 1, 0], np.float32), (len(p), 1))
    uv = np.stack([xs + 0.5, zs + 0.5], -1).reshape(-1, 2).astype(np.float32)
    idx = []
    for j in range(nz):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i, (j + 1) * (nx + 1) + i + 1
            idx += [a, c, b, b, c, d]
    return p, n, uv, np.array(idx, np.uint32)


def waving_cloth(rest, frame, amplitude=0.08):
    """The cloth's positions and normals at `frame`: a travelling wave along x (normals from the height field's gradient)."""
    x, z = rest[:, 0].astype(np.float64), rest[:, 2].astype(np.float64)
    ph = 0.6 * frame
    h = amplitude * np.sin(6.0 * x + ph) * np.cos(4.0 * z + 0.5 * ph)
    dx = amplitude * 6.0 * np.cos(6.0 * x + ph) * np.cos(4.0 * z + 0.5 * ph)
    dz = -amplitude * 4.0 * np.sin(6.0 * x + ph) * np.sin(4.0 * z + 0.5 * ph)
    p = rest.astype(np.float64).copy()
    p[:, 1] += h
    n = np.stack([-dx, np.ones_like(dx), -dz], -1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(np.float32), n.astype(np.float32)


def folded_cloth(rest, fold=1.0, gap=0.02):
    """The cloth folded onto itself along its middle line x = 0: the half x > 0 is turned about the z axis by `fold` x 180 degrees (fold 1:
    it lies `gap` above the other half, triangles that were a cloth's width apart now on top of each other).  Positions and normals.
    What a refit handles badly: the bind-pose tree pairs neighbours of the FLAT sheet, whose boxes now overlap the other half's."""
    p = rest.astype(np.float64).copy()
    n = np.tile(np.array([0.0, 1.0, 0.0]), (len(p), 1))
    ang = math.pi * fold
    c, s = math.cos(ang), math.sin(ang)
    right = p[:, 0] > 0.0
    x, y = p[right, 0], p[right, 1]
    p[right, 0] = c * x - s * y
    p[right, 1] = s * x + c * y + gap * fold
    n[right] = [-s, c, 0.0]
    return p.astype(np.float32), n.astype(np.float32)


def pulsing_sphere(rest, frame):
    """The sphere's positions at `frame`: scaled by a pulse around its centre (the normals keep their directions)."""
    return (rest * np.float32(1.0 + 0.25 * math.sin(0.9 * frame))).astype(np.float32)


def bending_cylinder(rings=10, segs=12, radius=0.15, height=1.2):
    """A cylinder along +y built for two-bone skinning: positions, normals, uvs, indices, joint indices (uint16 x 4) and weights (x 4).
    Bottom vertices follow joint 0 alone, top ones joint 1 alone (single-joint vertices); in between the weights blend and do NOT sum to
    one exactly (0.95-1.05) - the skinning contract uses them as given."""
    p, n, uv, ji, jw = [], [], [], [], []
    for r in range(rings + 1):
        t = r / rings
        for s in range(segs + 1):
            a = 2 * math.pi * s / segs
            p.append((radius * math.cos(a), height * t, radius * math.sin(a)))
            n.append((math.cos(a), 0.0, math.sin(a)))
            uv.append((s / segs, t))
            if t <= 0.2:
                ji.append((0, 0, 0, 0)); jw.append((1.0, 0.0, 0.0, 0.0))
            elif t >= 0.8:
                ji.append((1, 2, 0, 0)); jw.append((1.0, 0.0, 0.0, 0.0))
            else:
                w1 = (t - 0.2) / 0.6
                ji.append((0, 1, 2, 0)); jw.append((1.0 - w1, w1 * (0.95 + 0.1 * (s % 3) / 2), 0.0, 0.0))
    idx = []
    for r in range(rings):
        for s in range(segs):
            a, b = r * (segs + 1) + s, r * (segs + 1) + s + 1
            c, d = a + segs + 1, b + segs + 1
            idx += [a, c, b, b, c, d]
    return (np.array(p, np.float32), np.array(n, np.float32), np.array(uv, np.float32), np.array(idx, np.uint32), np.array(ji, np.uint16),
            np.array(jw, np.float32))


def bend_joints(frame, origin=(0.0, 0.0, 0.0), height=1.2):
    """Three column-major joint matrices for `frame`: 0 = the root (a translation), 1 = bent about z at mid-height, 2 = a slight scale."""
    o = np.array(origin, np.float64)
    j0 = np.eye(4); j0[:3, 3] = o
    ang = 0.35 * math.sin(0.5 * frame)
    c, s = math.cos(ang), math.sin(ang)
    rot = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    pivot, back = np.eye(4), np.eye(4)
    pivot[1, 3], back[1, 3] = 0.5 * height, -0.5 * height
    j1 = j0 @ pivot @ rot @ back
    j2 = j0 @ np.diag([1.1, 1.0, 0.9, 1.0])
    return np.stack([m.T.reshape(-1) for m in (j0, j1, j2)]).astype(np.float32)


def skin_reference(bind_p, bind_n, ji, jw, joints):
    """numpy float32 restatement of the skinning contract (hikari_hip.h hk_skin_mesh, Bevy 0.9 skinning.wgsl), operation for operation."""
    J = joints.reshape(-1, 4, 4)  # [joint][column][row]
    w = jw.astype(np.float32)
    M = w[:, 0, None, None] * J[ji[:, 0]]
    for t in range(1, 4):
        M = M + w[:, t, None, None] * J[ji[:, t]]
    x, y, z = bind_p[:, 0:1], bind_p[:, 1:2], bind_p[:, 2:3]
    pos = ((M[:, 0, :3] * x + M[:, 1, :3] * y) + M[:, 2, :3] * z) + M[:, 3, :3]
    c0, c1, c2 = M[:, 0, :3], M[:, 1, :3], M[:, 2, :3]

    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)

    cx, cy, cz = cross(c1, c2), cross(c2, c0), cross(c0, c1)
    det = ((c2[:, 0] * cz[:, 0] + c2[:, 1] * cz[:, 1]) + c2[:, 2] * cz[:, 2])[:, None]
    cx, cy, cz = cx / det, cy / det, cz / det
    nrm = (cx * bind_n[:, 0:1] + cy * bind_n[:, 1:2]) + cz * bind_n[:, 2:3]
    return pos.astype(np.float32), nrm.astype(np.float32)


def morph_reference(base_p, base_n, dp, dn, weights):
    """numpy float32 restatement of the morph contract (hikari_hip.h hk_set_mesh_morph_targets), operation for operation: base, then the
    targets whose weight does not compare equal to zero in ascending index, each product rounded, then each sum.  dp / dn: [target][v][3]
    (dn None: the base normals as they are).  Returns (positions, normals)."""
    w = np.asarray(weights, np.float32).reshape(-1)
    pos, nrm = np.array(base_p, np.float32).reshape(-1, 3), np.array(base_n, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        for k in range(len(w)):
            if w[k] == 0:   # (+0 and -0; a NaN weight is active)
                continue
            pos = pos + w[k] * np.asarray(dp[k], np.float32).reshape(-1, 3)
            if dn is not None:
                nrm = nrm + w[k] * np.asarray(dn[k], np.float32).reshape(-1, 3)
    return pos.astype(np.float32), nrm.astype(np.float32)


def morph_targets(positions, normals, n_targets, seed=0, normal_deltas=True):
    """`n_targets` dense morph targets for a coil_ribbon / cloth_grid mesh, in turn a bulge along the normals, a twist about the y axis and
    per-vertex noise, each with its own scale and phase: (position deltas, normal deltas or None), [target][v][3] float32."""
    rng = np.random.default_rng(seed)
    p, n = positions.astype(np.float64), normals.astype(np.float64)
    span = max(float(np.ptp(p[:, 1])), float(np.ptp(p[:, 0])), 1e-3)
    t = (p[:, 1] - p[:, 1].min()) / span if np.ptp(p[:, 1]) > 0 else (p[:, 0] - p[:, 0].min()) / span
    dp, dn = np.zeros((n_targets,) + p.shape), np.zeros((n_targets,) + p.shape)
    for k in range(n_targets):
        scale, phase = 0.04 + 0.02 * (k % 5), 0.61 * k
        if k % 3 == 0:    # bulge
            lobe = np.sin(math.pi * t * (1 + k % 4) + phase)
            dp[k] = scale * lobe[:, None] * n
            dn[k] = 0.3 * np.cos(math.pi * t * (1 + k % 4) + phase)[:, None] * np.array([0.0, 1.0, 0.0])
        elif k % 3 == 1:  # twist about y, growing with height
            ang = scale * 4.0 * t * math.cos(phase)
            c, s = np.cos(ang), np.sin(ang)
            for src, out in ((p, dp), (n, dn)):
                out[k, :, 0] = c * src[:, 0] - s * src[:, 2] - src[:, 0]
                out[k, :, 2] = s * src[:, 0] + c * src[:, 2] - src[:, 2]
        else:             # noise
            dp[k] = scale * 0.5 * rng.standard_normal(p.shape)
            dn[k] = 0.1 * rng.standard_normal(p.shape)
    return dp.astype(np.float32), (dn.astype(np.float32) if normal_deltas else None)


def morph_weights(n_targets, frame, phase=0.0, mode="wave"):
    """Animated weights of `n_targets` targets at `frame`, float32.  "wave": every target swings between about -0.3 and 1.2 (weights are
    used as given), and the targets k with (k + frame) % 4 == 0 are EXACTLY zero; "none": all zero; "one": target frame % n alone; "all":
    none zero; "alternate": every other one zero."""
    k = np.arange(n_targets)
    w = (0.45 + 0.75 * np.sin(0.8 * frame + phase + 0.9 * k)) / np.sqrt(1.0 + n_targets / 4.0)
    w = np.where(w == 0, 0.125, w)
    if mode == "wave":
        w[(k + frame) % 4 == 0] = 0.0
    elif mode == "none":
        w[:] = 0.0
    elif mode == "one":
        w[k != frame % n_targets] = 0.0
    elif mode == "alternate":
        w[k % 2 == 1] = 0.0
    elif mode != "all":
        raise ValueError(f"unknown mode {mode!r}")
    return w.astype(np.float32)


def deforming_scene(base="yard", cloth=(12, 12)):
    """A scene with three deforming meshes on top of `base` ("yard": synthetic_scene beyond the LDS copy, "small": one that fits it):
    a waving cloth, a bending cylinder (skinned) and a pulsing emissive sphere.  Returns (SceneData with .builder, sun, meshes) where
    meshes maps "cloth" / "cylinder" / "sphere" to dict(id=builder mesh id, rest=positions, normals=..., + the skin of the cylinder)."""
    if base == "yard":
        scene, sun = synthetic_scene(n_boxes=20, n_spheres=5, n_emitters=2, sphere_rings=12, sphere_segs=16)
    else:
        scene, sun = synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    cp, cn, cuv, cidx = cloth_grid(*cloth, size=2.0)
    yp, yn, yuv, yidx, ji, jw = bending_cylinder()
    sp, sn, suv, sidx = _sphere(6, 8)
    meshes = dict(cloth=dict(id=b.add_mesh(cp, cn, cuv, cidx), rest=cp, normals=cn),
                  cylinder=dict(id=b.add_mesh(yp, yn, yuv, yidx), rest=yp, normals=yn, joints=ji, weights=jw),
                  sphere=dict(id=b.add_mesh(sp, sn, suv, sidx), rest=sp, normals=sn))
    cloth_mat = b.add_material(standard_material((0.7, 0.2, 0.2, 1.0), (0, 0, 0), 0.7, 0.0, 0.5))
    glow = b.add_material(standard_material((0.9, 0.9, 0.9, 1.0), (1.0, 0.8, 0.5), 1.0, 0.0, 0.5))
    b.add_instance(meshes["cloth"]["id"], cloth_mat, _trs((0.5, 1.2, 0.3), (0.2, 0.4, 0.0), (1.0, 1.0, 1.0)))
    b.add_instance(meshes["cylinder"]["id"], cloth_mat, _trs((-1.0, 0.0, 0.8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    b.add_instance(meshes["sphere"]["id"], glow, _trs((1.2, 2.0, -0.6), (0.0, 0.0, 0.0), (0.4, 0.4, 0.4)))
    scene = b.finish()
    scene.builder = b
    for m in meshes.values():
        m["index"] = b.mesh_index(m["id"])
    return scene, sun, meshes


def large_cloth(triangles=1_000_000, size=2.0):
    """One cloth grid of about `triangles` triangles (tools/deform_probe.py: 10^4 - 10^6): positions, normals, uvs, indices."""
    side = max(2, int(round((triangles / 2) ** 0.5)))
    return cloth_grid(side, side, size=size)


# ---------------------------------------------------------------------------------------------
# a crowd of deforming meshes (hk_deform_meshes): many small meshes, each with its own motion
# ---------------------------------------------------------------------------------------------
def coil_ribbon(triangles, turns=1.5, radius=0.22, height=0.9, width=0.12):
    """A ribbon of exactly `triangles` triangles (triangles + 2 vertices) wound round the y axis: positions, outward normals, uvs, indices."""
    nv = triangles + 2
    steps = max((nv - 1) // 2, 1)
    p, n, uv = [], [], []
    for i in range(nv):
        t = (i // 2) / steps
        a = 2.0 * math.pi * turns * t
        p.append((radius * math.cos(a), height * t + width * (i % 2), radius * math.sin(a)))
        n.append((math.cos(a), 0.0, math.sin(a)))
        uv.append((t, float(i % 2)))
    idx = []
    for i in range(triangles):
        idx += [i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2]
    return np.array(p, np.float32), np.array(n, np.float32), np.array(uv, np.float32), np.array(idx, np.uint32)


def ribbon_skin(positions, n_joints, height=0.9):
    """Joint indices (uint16 x 4) and weights (x 4) of a coil_ribbon for a chain of `n_joints` joints along y: every vertex follows the
    two joints nearest its height, with weights that need not sum to one exactly (the skinning contract uses them as given)."""
    y = np.clip(positions[:, 1].astype(np.float64) / height, 0.0, 1.0) * (n_joints - 1)
    lo = np.minimum(np.floor(y).astype(np.int64), max(n_joints - 2, 0))
    hi = np.minimum(lo + 1, n_joints - 1)
    f = y - lo
    ji = np.zeros((len(positions), 4), np.uint16)
    jw = np.zeros((len(positions), 4), np.float32)
    ji[:, 0], ji[:, 1] = lo, hi
    jw[:, 0], jw[:, 1] = 1.0 - f, f * (0.97 + 0.03 * (np.arange(len(positions)) % 3))
    if n_joints == 1:
        jw[:, 0], jw[:, 1] = 1.0, 0.0
    return ji, jw


def chain_joints(n_joints, frame, phase=0.0, height=0.9):
    """`n_joints` column-major joint matrices at `frame`: joint k sways about z and x around its own height and stretches a little."""
    out = []
    for k in range(n_joints):
        t = k / max(n_joints - 1, 1)
        az = 0.30 * t * math.sin(0.5 * frame + phase + 0.7 * k)
        ax = 0.20 * t * math.cos(0.4 * frame + 1.3 * phase)
        cz, sz, cx, sx = math.cos(az), math.sin(az), math.cos(ax), math.sin(ax)
        rz = np.array([[cz, -sz, 0, 0], [sz, cz, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
        rx = np.array([[1, 0, 0, 0], [0, cx, -sx, 0], [0, sx, cx, 0], [0, 0, 0, 1]], np.float64)
        pivot, back = np.eye(4), np.eye(4)
        pivot[1, 3], back[1, 3] = height * t, -height * t
        m = pivot @ rz @ rx @ np.diag([1.0 + 0.05 * math.sin(0.3 * frame + k), 1.0, 1.0 - 0.04 * math.cos(0.2 * frame + phase), 1.0]) @ back
        m[0, 3] += 0.03 * math.sin(0.6 * frame + phase)
        out.append(m.T.reshape(-1))
    return np.stack(out).astype(np.float32)


def swaying_ribbon(rest, normals, frame, phase=0.0, height=0.9):
    """A coil_ribbon's positions and normals at `frame`: bent sideways more the higher up, breathing in and out."""
    p = rest.astype(np.float64).copy()
    t = p[:, 1] / height
    breathe = 1.0 + 0.15 * math.sin(0.7 * frame + phase)
    p[:, 0] = p[:, 0] * breathe + 0.25 * t * t * math.sin(0.5 * frame + phase)
    p[:, 2] = p[:, 2] * breathe + 0.15 * t * t * math.cos(0.4 * frame + 2.0 * phase)
    n = normals.astype(np.float64).copy()
    n[:, 1] = -0.3 * t * math.sin(0.5 * frame + phase)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return p.astype(np.float32), n.astype(np.float32)


def crowd_scene(base, sizes, joints=(1, 3, 17), n_emissive=2, n_doubled=3, extent=3.2, skinned=None):
    """A crowd on top of `base` ("yard" / "small", as deforming_scene): one coil_ribbon of sizes[k] triangles per entry, one instance each
    and a second one of `n_doubled` of them; `n_emissive` of the meshes glow.  Entries for which skinned(k) holds (default: the even ones)
    are skinned - palettes of `joints` joints in turn - the others are vertex-updated, every third of those without new normals.  Returns (SceneData with .builder, sun, meshes) like
    deforming_scene: meshes maps "m0", "m1", ... to dict(id, index, rest, normals, kind = "skin" / "vertices", pose = frame -> what the
    deformation call takes after the mesh: (joints,) or (positions, normals_or_None); skinned ones also joints / weights for
    set_mesh_skin) in the order the meshes were added."""
    if base == "yard":
        scene, sun = synthetic_scene(n_boxes=20, n_spheres=5, n_emitters=2, sphere_rings=12, sphere_segs=16)
    else:
        scene, sun = synthetic_scene(n_boxes=2, n_spheres=1, n_emitters=1, sphere_rings=4, sphere_segs=5)
    b = scene.builder
    n = len(sizes)
    plain = b.add_material(standard_material((0.3, 0.6, 0.8, 1.0), (0, 0, 0), 0.6, 0.0, 0.5))
    glow = b.add_material(standard_material((0.9, 0.9, 0.9, 1.0), (0.6, 1.0, 0.7), 1.0, 0.0, 0.5))
    emissive = {(j + 1) * n // (n_emissive + 1) for j in range(n_emissive)} if n else set()
    doubled = {(2 * j + 1) * n // (2 * n_doubled) for j in range(n_doubled)} if n else set()
    side = max(int(math.ceil(math.sqrt(n))), 1)
    meshes, vertex_items, skin_items = {}, 0, 0
    skinned = skinned or (lambda k: k % 2 == 0)
    for k, triangles in enumerate(sizes):
        p, nr, uv, idx = coil_ribbon(triangles)
        m = dict(id=b.add_mesh(p, nr, uv, idx), rest=p, normals=nr)
        phase = 0.37 * k
        if skinned(k):
            nj = joints[skin_items % len(joints)]
            skin_items += 1
            ji, jw = ribbon_skin(p, nj)
            m.update(kind="skin", joints=ji, weights=jw, pose=lambda frame, nj=nj, phase=phase: (chain_joints(nj, frame, phase),))
        else:
            keep_normals = vertex_items % 3 == 2
            vertex_items += 1

            def pose(frame, p=p, nr=nr, phase=phase, keep_normals=keep_normals):
                q, qn = swaying_ribbon(p, nr, frame, phase)
                return q, (None if keep_normals else qn)

            m.update(kind="vertices", pose=pose)
        gx, gz = k % side, k // side
        x, z = ((gx + 0.5) / side - 0.5) * 2.0 * extent, ((gz + 0.5) / side - 0.5) * 2.0 * extent
        b.add_instance(m["id"], glow if k in emissive else plain, _trs((x, 0.05, z), (0.0, 0.9 * k, 0.0), (1.0, 1.0, 1.0)))
        if k in doubled:
            b.add_instance(m["id"], plain, _trs((x + 0.3, 1.3, z - 0.2), (0.3, 0.5 * k, 0.1), (0.7, 0.8, 0.7)))
        meshes[f"m{k}"] = m
    scene = b.finish()
    scene.builder = b
    for m in meshes.values():
        m["index"] = b.mesh_index(m["id"])
    return scene, sun, meshes


def crowd_items(meshes, frame):
    """Engine.deform_meshes' item list for every mesh of a crowd_scene at `frame`, in the order the meshes were added."""
    return [(m["kind"], m["index"]) + tuple(m["pose"](frame)) for m in meshes.values()]
